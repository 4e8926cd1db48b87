"""GPU: the tail of a training step that turns gradients into new weights, element by element: tr_hyper_kernel
(rldm_train_hyper_step), tr_adamw_kernel (rldm_train_adamw, rldm_train_adamw_dyn), tr_sqnorm_kernel, tr_mse_kernel
(rangeldm_amd/csrc/train.hip).

Every reference below is a plain fp64 restatement of the formula the kernel cites, evaluated on the fp32 operands and the fp32
scalars the kernel receives (NOT training.cosine_lr / training.ema_decay, the project's other implementation of two of them):
  torch.optim.AdamW, decoupled weight decay:  p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
                                              p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
  clip_grad_norm_:                            g *= min(max_norm / (norm + 1e-6), 1)
  diffusers get_scheduler("cosine"):          lr * k / max(1, warmup)  for k < warmup, else
                                              lr * max(0, (1 + cos(pi (k - warmup) / max(1, total - warmup))) / 2),  k = step - 1
  diffusers EMAModel.get_decay(use_ema_warmup): 0 for step <= 1, else clamp(1 - (1 + (step - 1) / inv_gamma)^-power, 0, max_decay)
  diffusers EMAModel.step:                    ema -= (1 - decay) (ema - p)
All comparisons are per element; every buffer a kernel writes sits between two guards of 64 sentinel floats."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from tests.hip_util import _ulps

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = float(np.float32(-12345.678))
U = 2.0 ** -24                                   # the largest relative error of one fp32 rounding (half an ulp)


def f32(x):
    """the fp32 value a C float field holds for x, as a Python float"""
    return float(np.float32(x))


def ulp32(x):
    """fp32 unit in the last place at |x| (fp64 array in, fp64 out)"""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def guarded(vals, dtype=torch.float32, sent=SENT):
    """-> (buf, view): vals (cpu, 1-D) on the device between two guards of GUARD sentinels"""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n]
    view.copy_(vals.to(dtype))
    return buf, view


def assert_guards(buf, what, sent=SENT):
    b = buf.cpu()
    n = b.numel() - 2 * GUARD
    s = torch.full((GUARD,), sent, dtype=b.dtype)
    bits = {torch.float32: torch.int32, torch.float64: torch.int64}.get(b.dtype, b.dtype)
    assert torch.equal(b[:GUARD].view(bits), s.view(bits)), f"{what}: written before its first element"
    assert torch.equal(b[GUARD + n:].view(bits), s.view(bits)), f"{what}: written past its last element"


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def worst(x, ref, bound):
    """-> (largest |x - ref| / bound, its index); a non-finite x counts as inf"""
    x = x.double().numpy()
    r = np.abs(x - ref) / bound
    r = np.where(np.isfinite(x), r, np.inf)
    i = int(np.argmax(r))
    return float(r[i]), i


# ---- 1. hyper_step ----------------------------------------------------------------------------------------------------------------------
def ref_lr(step, lr, warmup, total):
    """diffusers get_cosine_schedule_with_warmup (num_cycles 0.5) after step - 1 scheduler steps, times the base rate"""
    k = step - 1
    if k < warmup:
        return lr * (float(k) / float(max(1, warmup)))
    progress = float(k - warmup) / float(max(1, total - warmup))
    return lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def ref_decay(step, inv_gamma, power, max_decay):
    """diffusers EMAModel.get_decay(optimization_step=step), use_ema_warmup=True, update_after_step 0, min_decay 0"""
    es = max(0, step - 1)
    if es <= 0:
        return 0.0
    return max(min(1.0 - (1.0 + es / inv_gamma) ** -power, max_decay), 0.0)


def ref_dyn(step, lr, betas, ema, warmup, total):
    """fp64 (lr, 1 - b1^step, 1 - b2^step, ema decay) of optimizer step `step`; lr, betas, ema: the fp32 values of the config"""
    return (ref_lr(step, lr, warmup, total), 1.0 - betas[0] ** step, 1.0 - betas[1] ** step, ref_decay(step, *ema))


LR0, BETAS = f32(1e-4), (f32(0.95), f32(0.999))
LR_CFGS = [(0, 10 ** 6), (1, 40), (3, 40), (500, 100000), (40, 40), (50, 40)]
EMA_CFGS = [(1.0, 0.75, 0.9999), (1.0, 2.0 / 3.0, 0.9999), (10.0, 0.75, 0.5)]
DYN_NAMES = ("lr", "bias correction 1", "bias correction 2", "ema decay")


def s0_values(warmup, total):
    s = {0, 1, 2, warmup - 1, warmup, warmup + 1, total - 2, total - 1, total, total + 7, 299999, 2 ** 31 + 2}
    return sorted(v for v in s if v >= 0)


def hyper_once(T, s0, ema, warmup, total, calls=1):
    """counter <- s0, `calls` hyper_steps -> (counter after, dyn[8] after each call); the counter sits between two int64 sentinels"""
    cnt = torch.tensor([-77, s0, -77], dtype=torch.int64, device="cuda")
    dyn = torch.full((8,), SENT, dtype=torch.float32, device="cuda")
    out = []
    for _ in range(calls):
        T.hyper_step(cnt[1:2], dyn, LR0, BETAS, ema[2], ema[0], ema[1], warmup, total)
        out.append(dyn.cpu().clone())
    c = cnt.cpu()
    assert c.dtype == torch.int64 and int(c[0]) == -77 and int(c[2]) == -77, "the words next to the step counter changed"
    return int(c[1]), out


@pytest.mark.parametrize("ema", EMA_CFGS, ids=lambda e: "ema%g-%.2f-%g" % e)
@pytest.mark.parametrize("warmup,total", LR_CFGS)
def test_hyper_step_matches_fp64_formulas(warmup, total, ema):
    """the four scalars of optimizer step s0 + 1 within 1 fp32 ulp of float32(fp64 formula) (the kernel computes in double and rounds
    once; device and host pow / cos may differ in the last double bits), the values that must be exact, the counter, dyn[4:8]."""
    from rangeldm_amd import train_ops as T
    ema32 = tuple(f32(v) for v in ema)
    sent = torch.full((4,), SENT)
    worst_ulps, bad = [0.0] * 4, []
    for s0 in s0_values(warmup, total):
        cnt, dyns = hyper_once(T, s0, ema32, warmup, total, calls=2)
        if cnt != s0 + 2:
            bad.append(f"s0={s0}: counter {cnt} after two calls, not {s0 + 2}")
        for call, dyn in enumerate(dyns):
            step = s0 + 1 + call
            what = f"s0={s0} call {call + 1} (step {step})"
            if not bits_equal(dyn[4:], sent):
                bad.append(f"{what}: dyn[4:8] written: {dyn[4:].tolist()}")
            ref = ref_dyn(step, LR0, BETAS, ema32, warmup, total)
            for j in range(4):
                ul = _ulps(dyn[j:j + 1], torch.tensor([f32(ref[j])], dtype=torch.float32))
                worst_ulps[j] = max(worst_ulps[j], ul)
                if not ul <= 1:
                    bad.append(f"{what}: {DYN_NAMES[j]} {float(dyn[j])!r} vs {f32(ref[j])!r} ({ul:g} ulps)")
            k = step - 1
            if step == 1 and warmup > 0 and float(dyn[0]) != 0.0:
                bad.append(f"{what}: lr {float(dyn[0])!r} at step 1 of a warmup, not 0")
            if k == warmup and float(dyn[0]) != LR0:
                bad.append(f"{what}: lr {float(dyn[0])!r} at k == warmup, not {LR0!r}")
            if step == 1 and float(dyn[3]) != 0.0:
                bad.append(f"{what}: ema decay {float(dyn[3])!r} at step 1, not 0")
            if step > 1 and 1.0 - (1.0 + (step - 1) / ema32[0]) ** -ema32[1] >= ema32[2] and float(dyn[3]) != ema32[2]:
                bad.append(f"{what}: ema decay {float(dyn[3])!r} under the clamp, not {ema32[2]!r}")
    print(f"hyper_step warmup={warmup} total={total} ema={ema}: worst ulps " +
          ", ".join(f"{n} {u:g}" for n, u in zip(DYN_NAMES, worst_ulps)))
    assert not bad, f"{len(bad)} mismatches: " + "; ".join(bad[:6])


def test_hyper_step_cases_reach_every_branch():
    """the chosen s0 reach the clamp of every EMA configuration and both sides of the warmup / cosine / span-guard branches, and
    the project's host formulas (training.cosine_lr, training.ema_decay) agree with the fp64 restatement used here."""
    from rangeldm_amd import training
    for ig, pw, md in ((f32(a), f32(b), f32(c)) for a, b, c in EMA_CFGS):
        clamped = [s for s in (299999, 2 ** 31 + 2) if 1.0 - (1.0 + s / ig) ** -pw >= md]
        free = [s for s in (1, 2) if 1.0 - (1.0 + s / ig) ** -pw < md]
        assert clamped and free, (ig, pw, md)
    for warmup, total in LR_CFGS:
        for s0 in s0_values(warmup, total):
            step = s0 + 1
            assert math.isclose(training.cosine_lr(step - 1, LR0, warmup, total), ref_lr(step, LR0, warmup, total), rel_tol=1e-15,
                                abs_tol=0.0), (warmup, total, s0)
            for ig, pw, md in EMA_CFGS:
                assert training.ema_decay(step, md, ig, pw) == ref_decay(step, ig, pw, md), (step, ig, pw, md)


# ---- 2. adamw / adamw_dyn ---------------------------------------------------------------------------------------------------------------
# Per-element bounds, from the kernel's operation count (u = 2^-24: one fp32 rounding moves a value by at most u relative, half an ulp).
#   exp_avg     m = fl(fl(b1 m0) + fl((1 - b1) g)): three roundings; where the two terms agree in sign that is <= 2 u |m| < 3 ulp(m).
#   exp_avg_sq  v = fl(fl(b2 v0) + fl(fl((1 - b2) g) g)): four roundings of positive terms, <= 3 u v <= 3 ulp(v).
#   parameters  fl(p fl(1 - lr wd)) - fl(fl(lr / bc1) fl(m / fl(fl(sqrtf(v) / sqrtf(bc2)) + eps))): 1.5 ulp(p) from the decay factor,
#               the product and the last subtraction (<= 2 ulp); the update carries m (2 u), sqrt v (1.5 u), two square roots, two
#               divisions, the sum with eps, lr / bc1 and the product: 10.5 u < 2^-20 = 16 u.
#   EMA         fl(ema - fl(fl(1 - d) fl(ema - p))): 3 u of the increment and half an ulp of the result.
# Two things the 3-ulp bounds on m and v leave out, and that the fp64 reference alone shows (neither looks at the kernel's output):
#   * cancellation: at a later step b1 m0 and (1 - b1) g have either sign, and where they cancel, m is small against the two roundings
#     that made it.  The rounding error is <= u (|a| + |b| + |m|) = 2 u |m| + u c with c = |a| + |b| - |m|; the bound gets 2 u c.
#   * the clipping coefficient, which the kernel computes in fp32: (float) sqrt(sq), + 1e-6f, the division: 3 u, and fl(g coef) one
#     more: g carries 4 u.  m gets 4 u |(1 - b1) g|, v gets 8 u (1 - b2) g^2.  Both vanish when the coefficient is exactly 1.
# What m and v may be off beyond 3 ulps reaches the parameters through the update (dm / denom and |update| dv / 2 v), and whatever the
# parameters may be off reaches the EMA times (1 - d): EMAModel.step reads the NEW parameters.
# Largest observed |x - ref| / bound on an MI355X over every case of test_adamw_per_element (all must be <= 1):
#   exp_avg 0.491, exp_avg_sq 0.491, parameters 0.364, EMA 0.270 (test_hyper_adamw_chain, against its summed bounds: 0.207, 0.363,
#   0.226, 0.177).  Elsewhere in this file: hyper_step 0 ulps on every value of every case (bound 1), sqnorm 1.4e-15 relative (bound
#   1e-13), mse dpred 0.50 ulps (bound 2) and loss 2e-16 relative (bound 1e-13).
M_ULPS, V_ULPS, P_ULPS, UPD_REL = 3.0, 3.0, 2.0, 2.0 ** -20
HP = dict(lr=f32(1e-3), b1=f32(0.95), b2=f32(0.999), eps=f32(1e-8), wd=f32(1e-2))
CLIP_CASES = ("none", "off", "half", "three", "one")
SIZES = (1, 255, 256, 257, 10007, 2 ** 20 + 3)


def adamw_ref(p, g, m0, v0, e0, lr, bc1, bc2, decay, sq, max_norm, Bm0=0.0, Bv0=0.0):
    """One AdamW + clip + EMA step in fp64 (numpy fp64 arrays of the fp32 operands; fp64 scalars of the fp32 values the kernel gets;
    sq: the squared gradient norm the kernel is handed, or None) -> dict(m, v, p, e) and the bounds bm, bv, bp, be on what a correct
    fp32 kernel may differ by.  Bm0 / Bv0: what the m0 / v0 the kernel starts from may already differ by (a chain of steps)."""
    b1, b2, eps, wd = HP["b1"], HP["b2"], HP["eps"], HP["wd"]
    coef = 1.0
    if sq is not None and max_norm > 0:
        coef = min(max_norm / (math.sqrt(sq) + 1e-6), 1.0)
    eg = 4 * U if coef < 1.0 else 0.0
    gs = g * coef
    a, b = b1 * m0, (1.0 - b1) * gs
    m = a + b
    bq = (1.0 - b2) * gs * gs
    v = b2 * v0 + bq
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    upd = (lr / bc1) * (m / denom)
    pn = p * (1.0 - lr * wd) - upd
    xm = 2 * U * (np.abs(a) + np.abs(b) - np.abs(m)) + eg * np.abs(b) + b1 * Bm0
    xv = 2 * eg * bq + b2 * Bv0
    bm, bv = M_ULPS * ulp32(m) + xm, V_ULPS * ulp32(v) + xv
    bp = P_ULPS * ulp32(pn) + UPD_REL * np.abs(upd) + (lr / bc1) * xm / denom + np.abs(upd) * xv / (2 * np.maximum(v, 1e-300))
    out = dict(m=m, v=v, p=pn, bm=bm, bv=bv, bp=bp, upd=upd, coef=coef)
    if e0 is not None:
        inc = (1.0 - decay) * (e0 - pn)
        out["e"] = e0 - inc
        out["inc"] = inc
        out["be"] = P_ULPS * ulp32(out["e"]) + UPD_REL * np.abs(inc)          # + (1 - decay) * (what p is off by): the caller's
    return out


def adamw_operands(n, clip, step):
    """fp32 cpu operands (p, g, m0, v0, e0), the squared norm handed to the kernel (python float or None) and max_grad_norm"""
    p = rnd(n, 1)
    e0 = p + 0.01 * rnd(n, 2)
    if step == 1:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:
        m0, v0 = 1e-3 * rnd(n, 3), 1e-6 * rnd(n, 4) ** 2
    g = rnd(n, 5)
    norm = float(g.double().norm())
    if clip == "one":
        g = torch.zeros(n)
        g[n - 1] = 1.0
    elif clip == "half":
        g = (g.double() * (0.5 / norm)).float()
    else:
        g = (g.double() * (3.0 / norm)).float()
    sq = None if clip == "none" else float((g.double() ** 2).sum())
    if clip == "one":
        assert sq == 1.0
    return p, g, m0, v0, e0, sq, (0.0 if clip == "off" else 1.0)


def step_scalars(step):
    """fp32 (lr, bc1, bc2, decay) of optimizer step `step`, as rldm_train_adamw derives them from its config on the host"""
    return (HP["lr"], f32(1.0 - HP["b1"] ** step), f32(1.0 - HP["b2"] ** step), f32(ref_decay(step, 1.0, 0.75, f32(0.9999))))


def run_adamw(T, entry, ops, step, with_ema, zero_grads):
    """one launch on fresh guarded copies -> dict of cpu results"""
    p, g, m0, v0, e0, sq, max_norm = ops
    lr, bc1, bc2, decay = step_scalars(step)
    bufs = {k: guarded(t) for k, t in (("p", p), ("g", g), ("m", m0), ("v", v0))}
    if with_ema:
        bufs["e"] = guarded(e0)
    sqb = None
    if sq is not None:
        sqb = guarded(torch.tensor([sq], dtype=torch.float64), torch.float64, -7.5)
    ema = bufs["e"][1] if with_ema else None
    kw = dict(ema=ema, sqnorm_dev=None if sqb is None else sqb[1], max_grad_norm=max_norm)
    betas = (HP["b1"], HP["b2"])
    if entry == "adamw":
        T.adamw(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], step, lr, betas, HP["eps"], HP["wd"], ema_decay=decay, **kw)
    else:
        dyn = torch.full((8,), SENT, dtype=torch.float32, device="cuda")
        dyn[:4] = torch.tensor([lr, bc1, bc2, decay], dtype=torch.float32)
        T.adamw_dyn(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], dyn, betas, HP["eps"], HP["wd"], zero_grads=zero_grads, **kw)
        d = dyn.cpu()
        assert bits_equal(d[:4], torch.tensor([lr, bc1, bc2, decay], dtype=torch.float32)) and bits_equal(d[4:], torch.full((4,), SENT))
    torch.cuda.synchronize()
    what = f"{entry} zero_grads={zero_grads} ema={with_ema}"
    for k, (buf, _) in bufs.items():
        assert_guards(buf, f"{what}: buffer {k}")
    if sqb is not None:
        assert_guards(sqb[0], f"{what}: sqnorm", -7.5)
        assert float(sqb[1].cpu()) == sq, f"{what}: the squared norm was overwritten"
    return {k: view.cpu() for k, (_, view) in bufs.items()}


@pytest.mark.parametrize("clip", CLIP_CASES)
@pytest.mark.parametrize("n", SIZES)
def test_adamw_per_element(n, clip):
    """rldm_train_adamw and rldm_train_adamw_dyn (zero_grads on / off), with and without an EMA, at step 1 (zero moments) and step 7
    (prefilled moments), against the fp64 recurrences: exp_avg, exp_avg_sq, parameters and EMA per element, the gradient buffer
    (cleared to +0.0 or untouched bit for bit), the guards, and the two entry points bit for bit against each other."""
    from rangeldm_amd import train_ops as T
    ratios = dict(m=0.0, v=0.0, p=0.0, e=0.0)
    bad = []
    for step in (1, 7):
        ops = adamw_operands(n, clip, step)
        p, g, m0, v0, e0, sq, max_norm = ops
        lr, bc1, bc2, decay = step_scalars(step)
        ref = adamw_ref(*(t.double().numpy() for t in (p, g, m0, v0, e0)), lr, bc1, bc2, decay, sq, max_norm)
        if clip == "one":
            assert ref["coef"] == 1.0 / (1.0 + 1e-6)
        elif clip in ("none", "off", "half"):
            assert ref["coef"] == 1.0
        else:
            assert 0.33 < ref["coef"] < 0.34
        for with_ema in (False, True):
            first = None
            for entry, zg in (("adamw", False), ("adamw_dyn", False), ("adamw_dyn", True)):
                what = f"step {step} {entry} zero_grads={zg} ema={with_ema}"
                out = run_adamw(T, entry, ops, step, with_ema, zg)
                if zg:
                    if not bits_equal(out["g"], torch.zeros(n)):
                        bad.append(f"{what}: the gradient buffer is not all +0.0")
                elif not bits_equal(out["g"], g):
                    bad.append(f"{what}: the gradient buffer changed")
                bounds = dict(m=ref["bm"], v=ref["bv"], p=ref["bp"])
                if with_ema:
                    bounds["e"] = ref["be"] + (1.0 - decay) * ref["bp"]
                for k, bound in bounds.items():
                    r, i = worst(out[k], ref[k], bound)
                    ratios[k] = max(ratios[k], r)
                    if not r <= 1.0:
                        bad.append(f"{what}: {k}[{i}] = {float(out[k][i])!r} vs {float(ref[k][i])!r}, {r:.3g} x its bound")
                if first is None:
                    first = out
                else:
                    for k in bounds:
                        if not bits_equal(out[k], first[k]):
                            bad.append(f"{what}: {k} differs from rldm_train_adamw's on the same fp32 scalars")
    print(f"adamw n={n} clip={clip}: worst |x - ref| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    assert not bad, f"{len(bad)} mismatches: " + "; ".join(bad[:6])


# ---- 3. sqnorm --------------------------------------------------------------------------------------------------------------------------
def sqnorm_into(g, out_view):
    _lib.check(_lib.lib().rldm_train_sqnorm(C.c_void_p(g.data_ptr()), g.numel(), C.c_void_p(out_view.data_ptr()),
                                            _lib.stream_ptr(g.device)), "rldm_train_sqnorm")
    torch.cuda.synchronize()
    return float(out_view.cpu())


@pytest.mark.parametrize("n", [1, 257, 65536, 3 * 2 ** 20 + 5])       # the launch caps its grid at 2048 blocks: 256 * 2048 < 3 * 2^20 + 5
def test_sqnorm_fp64_sum(n):
    """within 1e-13 relative of the fp64 sum of squares (each product of two fp32 values is exact in fp64: only the order of the
    sum differs); the same value on a second call into the same accumulator; inf for a buffer that holds one inf."""
    g = rnd(n, 11)
    ref = math.fsum((g.double() ** 2).tolist())
    gbuf, gv = guarded(g)
    obuf, ov = guarded(torch.tensor([1e300], dtype=torch.float64), torch.float64, -7.5)
    first = sqnorm_into(gv, ov)
    second = sqnorm_into(gv, ov)
    print(f"sqnorm n={n}: relative error {abs(first - ref) / ref:.3g}, second call {abs(second - ref) / ref:.3g}")
    assert abs(first - ref) <= 1e-13 * ref, (first, ref)
    assert abs(second - ref) <= 1e-13 * ref, f"second call into the same accumulator: {second!r} (first {first!r})"
    assert_guards(obuf, "sqnorm accumulator", -7.5)
    assert_guards(gbuf, "sqnorm input")
    assert bits_equal(gv.cpu(), g)
    from rangeldm_amd import train_ops as T
    assert abs(float(T.sqnorm(gv)) - ref) <= 1e-13 * ref
    gv[n // 2] = float("inf")
    got = sqnorm_into(gv, ov)
    assert math.isinf(got) and got > 0, got


# ---- 4. mse -----------------------------------------------------------------------------------------------------------------------------
MSE_WEIGHTS = {3: [None, (0.5, 1.0, 0.25), (0.5, 0.0, 0.25)], 1: [None, (0.5,), (0.0,)], 2: [None, (0.5, 1.0), (0.0, 0.25)]}


@pytest.mark.parametrize("B,Cc,W,H", [(3, 5, 7, 2), (1, 4, 8, 4), (2, 4, 64, 8)])
def test_mse_per_element(B, Cc, W, H):
    """dpred within 2 fp32 ulps of w_b 2 d / total in fp64 from the fp32 difference d the kernel takes, the loss within 1e-13 of the
    fp64 sum, dpred == 0 for samples of weight 0.  pred is (B, W, H, C), target (B, C, W, H) with a value that differs under
    any swap of two of its axes, so a wrong index map on either side shows in every element."""
    from rangeldm_amd import train_ops as T
    total = B * Cc * W * H
    bb, cc, ww, hh = np.meshgrid(np.arange(B), np.arange(Cc), np.arange(W), np.arange(H), indexing="ij")
    target = ((bb + 10 * cc + 100 * ww + 1000 * hh) / 1024.0).astype(np.float32)              # exact in fp32
    pred = torch.randn(B, W, H, Cc, generator=torch.Generator().manual_seed(21)) * 4.0
    d = pred.numpy() - np.transpose(target, (0, 2, 3, 1))                                      # fp32 - fp32 in fp32, (B, W, H, C)
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    pbuf, pv = guarded(pred.reshape(-1))
    tbuf, tv = guarded(torch.from_numpy(target).reshape(-1))
    for wts in MSE_WEIGHTS[B]:
        w64 = np.ones(B) if wts is None else np.array([f32(w) for w in wts], dtype=np.float64)
        dref = w64[:, None, None, None] * 2.0 * d / total
        lref = math.fsum((w64[:, None, None, None] * d * d / total).reshape(-1).tolist())
        wd = None if wts is None else torch.tensor(wts, dtype=torch.float32, device="cuda")
        loss, dp = T.mse(pv.view(B, W, H, Cc), tv.view(B, Cc, W, H), wd)
        loss2, dp2 = T.mse(pv.view(B, W, H, Cc), tv.view(B, Cc, W, H), wd)
        dp, lv = dp.cpu(), float(loss)
        ul = _ulps(dp.reshape(-1), torch.from_numpy(dref).reshape(-1))
        print(f"mse {(B, Cc, W, H)} weights {wts}: dpred {ul:g} ulps, loss {lv!r} vs {lref!r}")
        assert dp.shape == (B, W, H, Cc)
        assert ul <= 2, f"weights {wts}: dpred {ul:g} ulps off"
        assert abs(lv - lref) <= 1e-13 * lref, (wts, lv, lref)
        assert abs(float(loss2) - lref) <= 1e-13 * lref and bits_equal(dp2.cpu(), dp), f"weights {wts}: a second call differs"
        for b in range(B):
            if w64[b] == 0:
                assert bool((dp[b] == 0).all()), f"weights {wts}: sample {b} has weight 0 and a gradient"
            else:
                assert bool((dp[b] != 0).any())
    assert_guards(pbuf, "mse pred")
    assert_guards(tbuf, "mse target")


# ---- 5. a short chain through both kernels ----------------------------------------------------------------------------------------------
def test_hyper_adamw_chain():
    """8 hyper_step + sqnorm + adamw_dyn(zero_grads=True) steps on n = 10007 with lr_warmup_steps 3 and total_steps 6 (across the warmup
    boundary, the end of the cosine and two steps past it), a fresh gradient each step, clipping and EMA on, against the fp64 loop.
    Errors add: the bound after step t is the sum of the per-step bounds of section 2 up to t, each evaluated on that step's
    reference values, with what exp_avg / exp_avg_sq are already off by carried into the next step's update."""
    from rangeldm_amd import train_ops as T
    n, warmup, total, steps = 10007, 3, 6, 8
    ema_cfg = (f32(1.0), f32(0.75), f32(0.9999))
    betas = (HP["b1"], HP["b2"])
    p0, e0 = rnd(n, 31), rnd(n, 31) + 0.01 * rnd(n, 32)
    bufs = {k: guarded(t) for k, t in (("p", p0), ("g", torch.zeros(n)), ("m", torch.zeros(n)), ("v", torch.zeros(n)), ("e", e0))}
    cnt = torch.tensor([-77, 0, -77], dtype=torch.int64, device="cuda")
    dyn = torch.full((8,), SENT, dtype=torch.float32, device="cuda")
    ref = dict(p=p0.double().numpy(), m=np.zeros(n), v=np.zeros(n), e=e0.double().numpy())
    B = dict(m=0.0, v=0.0, p=0.0, e=0.0)
    ratios = dict(m=0.0, v=0.0, p=0.0, e=0.0)
    bad = []
    for step in range(1, steps + 1):
        g = rnd(n, 40 + step)
        g = (g.double() * ((3.0 if step % 2 else 0.5) / float(g.double().norm()))).float()        # odd steps clip
        bufs["g"][1].copy_(g)
        sq_dev = T.sqnorm(bufs["g"][1])
        T.hyper_step(cnt[1:2], dyn, HP["lr"], betas, ema_cfg[2], ema_cfg[0], ema_cfg[1], warmup, total)
        T.adamw_dyn(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], dyn, betas, HP["eps"], HP["wd"], ema=bufs["e"][1],
                    sqnorm_dev=sq_dev, max_grad_norm=1.0, zero_grads=True)
        d, sq = dyn.cpu(), float(sq_dev)
        sq_ref = math.fsum((g.double() ** 2).tolist())
        assert abs(sq - sq_ref) <= 1e-13 * sq_ref, f"step {step}: sqnorm {sq!r} vs {sq_ref!r}"
        want = ref_dyn(step, HP["lr"], betas, ema_cfg, warmup, total)
        for j in range(4):
            ul = _ulps(d[j:j + 1], torch.tensor([f32(want[j])], dtype=torch.float32))
            assert ul <= 1, f"step {step}: {DYN_NAMES[j]} {float(d[j])!r} vs {f32(want[j])!r}"
        assert bits_equal(d[4:], torch.full((4,), SENT))
        # the recurrences on the scalars the kernel read (each within 1 ulp of its formula, asserted above)
        lr, bc1, bc2, decay = (float(x) for x in d[:4])
        r = adamw_ref(ref["p"], g.double().numpy(), ref["m"], ref["v"], ref["e"], lr, bc1, bc2, decay, sq, 1.0, Bm0=B["m"], Bv0=B["v"])
        B["m"], B["v"] = r["bm"], r["bv"]              # (adamw_ref already carried b1 Bm0 / b2 Bv0 into them)
        B["p"] = B["p"] + r["bp"]
        B["e"] = decay * B["e"] + r["be"] + (1.0 - decay) * B["p"]
        for k in ("m", "v", "p", "e"):
            ref[k] = r[k]
            x = bufs[k][1].cpu()
            ratio, i = worst(x, ref[k], B[k])
            ratios[k] = max(ratios[k], ratio)
            if not ratio <= 1.0:
                bad.append(f"step {step}: {k}[{i}] = {float(x[i])!r} vs {float(ref[k][i])!r}, {ratio:.3g} x its bound")
        if not bits_equal(bufs["g"][1].cpu(), torch.zeros(n)):
            bad.append(f"step {step}: the gradient buffer is not all +0.0")
    print("chain: worst |x - ref| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    c = cnt.cpu()
    assert c.tolist() == [-77, steps, -77], c.tolist()
    for k, (buf, _) in bufs.items():
        assert_guards(buf, f"chain buffer {k}")
    assert not bad, f"{len(bad)} mismatches: " + "; ".join(bad[:6])
