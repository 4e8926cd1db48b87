"""Helpers for the -m gpu parity tests (call librangeldm_hip through its C ABI)."""
import ctypes as C

import numpy as np
import torch

from rangeldm_amd import _lib


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _ulps(a, b):
    a, b = a.double(), b.double()
    ulp = torch.from_numpy(np.spacing(np.abs(b.numpy()).astype(np.float32)).astype(np.float64))
    return float(((a - b).abs() / ulp).max())


def hip_conv(x0, weight, bias, x1=None, stride=1, pad_mode=0, upsample=False, gamma=None, beta=None, silu=False,
             eps=1e-5, temb=None, res=None):
    """rldm_test_conv: fp32 NCHW tensors in/out, the kernel under test in the middle."""
    dev = torch.device("cuda")
    d = _lib.ConvDescC()
    B, C0, W, H = x0.shape
    d.B, d.Cin0, d.Win, d.Hin = B, C0, W, H
    d.Cin1 = 0 if x1 is None else x1.shape[1]
    d.Cout, d.ksize = weight.shape[0], weight.shape[2]
    d.stride, d.pad_mode, d.upsample = stride, pad_mode, 1 if upsample else 0
    d.gn, d.silu, d.eps = (1 if gamma is not None else 0), (1 if silu else 0), eps
    up = 2 if upsample else 1
    Wo, Ho = W * up // stride, H * up // stride
    y = torch.empty((B, d.Cout, Wo, Ho), device=dev, dtype=torch.float32)

    def devp(t):
        if t is None:
            return None, None
        t = t.to(dev, torch.float32).contiguous()
        return t, C.c_void_p(t.data_ptr())

    def hostp(t):
        if t is None:
            return None, None
        a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        return a, a.ctypes.data_as(C.c_void_p)

    k0, p0 = devp(x0)
    k1, p1 = devp(x1)
    kr, pr = devp(res)
    hw, pw = hostp(weight)
    hb, pb = hostp(bias)
    hg, pg = hostp(gamma)
    hbt, pbt = hostp(beta)
    ht, pt = hostp(temb)
    _lib.check(_lib.lib().rldm_test_conv(C.byref(d), p0, p1, pw, pb, pg, pbt, pt, pr, C.c_void_p(y.data_ptr()),
                                         _lib.stream_ptr(dev)), "rldm_test_conv")
    torch.cuda.synchronize()
    return y.cpu()


def hip_attention(qkv, C_):
    dev = torch.device("cuda")
    B, L, _ = qkv.shape
    q = qkv.to(dev, torch.float32).contiguous()
    out = torch.empty((B, L, C_), device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().rldm_test_attention(C.c_void_p(q.data_ptr()), B, L, C_, C.c_void_p(out.data_ptr()),
                                              _lib.stream_ptr(dev)), "rldm_test_attention")
    torch.cuda.synchronize()
    return out.cpu()


def hip_conv_stats(x0, weight, bias, stride=1):
    """rldm_test_conv_stats: per-image per-channel (sum, sumsq) the conv epilogue emitted for its bf16 output."""
    dev = torch.device("cuda")
    d = _lib.ConvDescC()
    B, C0, W, H = x0.shape
    d.B, d.Cin0, d.Win, d.Hin, d.Cin1 = B, C0, W, H, 0
    d.Cout, d.ksize = weight.shape[0], weight.shape[2]
    d.stride, d.pad_mode, d.upsample, d.gn, d.silu, d.eps = stride, 0, 0, 0, 0, 1e-5
    xs = x0.to(dev, torch.float32).contiguous()
    hw = np.ascontiguousarray(weight.numpy(), dtype=np.float32)
    hb = np.ascontiguousarray(bias.numpy(), dtype=np.float32)
    st = torch.empty((B, d.Cout, 2), device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().rldm_test_conv_stats(C.byref(d), C.c_void_p(xs.data_ptr()), hw.ctypes.data_as(C.c_void_p),
                                               hb.ctypes.data_as(C.c_void_p), C.c_void_p(st.data_ptr()),
                                               _lib.stream_ptr(dev)), "rldm_test_conv_stats")
    torch.cuda.synchronize()
    return st.cpu()


def hip_conv_sched(x0, weight, bias, gamma, beta, sampler_mode, prediction_type, coef_table, step, x, noise, noise_step_stride, x_prev,
                   pack=None, pack_ld=0, silu=True, eps=1e-5):
    """rldm_test_conv_sched: the 3x3 output layer conv(silu(GN(x0))) with the scheduler step in its epilogue, as a captured sampler runs
    it.  x0 fp32 NCHW and weight / bias / gamma / beta as hip_conv takes them; coef_table (float32 [rows][5]), step (int32 [1]), x,
    noise, x_prev (float32) and pack (int16 bit patterns of bf16, or None) are CUDA tensors used IN PLACE -- views are fine, their
    data_ptr is what the kernel gets (a lane's noise offset, x_prev aliasing x).  -> (eps on the device, name of the carrying launch)."""
    dev = torch.device("cuda")
    d = _lib.ConvDescC()
    B, C0, W, H = x0.shape
    d.B, d.Cin0, d.Cin1, d.Win, d.Hin = B, C0, 0, W, H
    d.Cout, d.ksize = weight.shape[0], weight.shape[2]
    d.stride, d.pad_mode, d.upsample = 1, 0, 0
    d.gn, d.silu, d.eps = (1 if gamma is not None else 0), (1 if silu else 0), eps
    for t, dt in ((coef_table, torch.float32), (step, torch.int32), (x, torch.float32), (x_prev, torch.float32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    assert noise is None or (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous())
    assert pack is None or (pack.is_cuda and pack.dtype == torch.int16 and pack.is_contiguous())
    s = _lib.ConvSchedDescC()
    s.sampler_mode, s.prediction_type = int(sampler_mode), int(prediction_type)
    s.coef_table, s.step, s.x, s.x_prev = coef_table.data_ptr(), step.data_ptr(), x.data_ptr(), x_prev.data_ptr()
    s.noise = noise.data_ptr() if noise is not None else None
    s.noise_step_stride = int(noise_step_stride)
    s.pack = pack.data_ptr() if pack is not None else None
    s.pack_ld = int(pack_ld)
    xs = x0.to(dev, torch.float32).contiguous()
    y = torch.empty((B, d.Cout, W, H), device=dev, dtype=torch.float32)

    def hostp(t):
        if t is None:
            return None, None
        a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        return a, a.ctypes.data_as(C.c_void_p)

    hw, pw = hostp(weight)
    hb, pb = hostp(bias)
    hg, pg = hostp(gamma)
    hbt, pbt = hostp(beta)
    name = C.create_string_buffer(128)
    _lib.check(_lib.lib().rldm_test_conv_sched(C.byref(d), C.c_void_p(xs.data_ptr()), pw, pb, pg, pbt, C.byref(s),
                                               C.c_void_p(y.data_ptr()), name, len(name), _lib.stream_ptr(dev)), "rldm_test_conv_sched")
    torch.cuda.synchronize()
    return y, name.value.decode()


def hip_temb_layout(model):
    """rldm_test_temb_layout of a finalized UNet2DModelHIP -> (ld, {resnet prefix: first column}), the prefixes in column order."""
    L = _lib.lib()
    v = C.c_int(0)
    _lib.check(L.rldm_test_temb_layout(model._h, None, C.byref(v)), "rldm_test_temb_layout")
    ld = v.value
    offs = {}
    for name in model._shapes:
        if name.endswith(".time_emb_proj.bias"):
            prefix = name[:-len(".time_emb_proj.bias")]
            _lib.check(L.rldm_test_temb_layout(model._h, prefix.encode(), C.byref(v)), "rldm_test_temb_layout")
            offs[prefix] = v.value
    return ld, dict(sorted(offs.items(), key=lambda kv: kv[1]))


def hip_temb(model, timesteps, ld=None):
    """rldm_test_temb: the time-embedding table of a finalized UNet2DModelHIP for `timesteps` (ints, any count >= 1), through the
    conversion and the launches rldm_unet_forward and the samplers use.  -> fp32 [n][ld] on the CPU (ld: hip_temb_layout's, if known)."""
    ts = np.ascontiguousarray(np.asarray(timesteps, dtype=np.int64).reshape(-1))
    if ld is None:
        ld = hip_temb_layout(model)[0]
    tab = torch.empty((len(ts), ld), device=model.device, dtype=torch.float32)
    _lib.check(_lib.lib().rldm_test_temb(model._h, ts.ctypes.data_as(C.c_void_p), len(ts), C.c_void_p(tab.data_ptr()),
                                         _lib.stream_ptr(model.device)), "rldm_test_temb")
    torch.cuda.synchronize()
    return tab.cpu()


def hip_attention_qkv(x, gamma, beta, wqkv, bqkv, groups=32, eps=1e-5):
    """rldm_test_attention_qkv: the fused GroupNorm -> q/k/v -> softmax.V launch of every UNet attention block.
    x (B, L, C) token-major fp32 -> (B, L, C) heads concatenated (before to_out)."""
    dev = torch.device("cuda")
    B, L, C_ = x.shape
    xs = x.to(dev, torch.float32).contiguous()
    out = torch.empty((B, L, C_), device=dev, dtype=torch.float32)

    def hostp(t):
        a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        return a, a.ctypes.data_as(C.c_void_p)

    hg, pg = hostp(gamma)
    hb, pb = hostp(beta)
    hw, pw = hostp(wqkv)
    hq, pq = hostp(bqkv)
    _lib.check(_lib.lib().rldm_test_attention_qkv(C.c_void_p(xs.data_ptr()), B, L, C_, groups, eps, pg, pb, pw, pq,
                                                  C.c_void_p(out.data_ptr()), _lib.stream_ptr(dev)),
               "rldm_test_attention_qkv")
    torch.cuda.synchronize()
    return out.cpu()


# ---- exact-operand testing ----------------------------------------------------------------------------------------------------------
# Operands that are small integers times a power of two are exact in bf16, every product of two of them is exact in fp32, and a sum of
# such products is exact in fp32 in ANY order (MFMA chains, k-groups, split-K atomics, partial-tile reductions) as long as the sum of
# the absolute values of its terms stays below 2^24 units of the finest grid.  A kernel then has exactly one right answer: the fp64
# reference, rounded once to the output type (bf16: round to nearest even, as common.h f32_to_bf16 and torch both do).
def int_grid(shape, seed, lo=-3, hi=3, exp=0, density=1.0):
    """Seeded integers in [lo, hi] times 2^exp (fp32); `density` < 1 zeroes the rest.  Exact in bf16 while max(|lo|, |hi|) <= 256."""
    assert max(abs(lo), abs(hi)) <= 256, "more than 8 significant bits: not exact in bf16"
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density).to(torch.float32)
    return v * 2.0 ** exp


def assert_on_grid(t, unit, bits=8):
    """every value of `t` is an integer multiple of `unit` with at most `bits` significant bits (bf16: 8)."""
    q = t.double().cpu() / unit
    assert torch.equal(q, q.round()), f"values off the {unit} grid"
    assert torch.equal(t.to(torch.bfloat16).to(t.dtype), t), "values not exact in bf16"


def assert_exact_bound(unit, *terms):
    """terms: (count, magnitude) pairs -- `count` addends of absolute value <= `magnitude`, all multiples of `unit`, summed into every
    output.  Asserts the fp32 sum is exact in any order (sum of |addends| < 2^24 units); -> that sum in units."""
    total = sum(float(n) * float(m) for n, m in terms) / unit
    assert total < 2 ** 24, f"the exactness bound does not hold: up to {total:.3g} units of {unit} (>= 2^24)"
    return total


def amax(*ts):
    return max(float(t.abs().max()) for t in ts if t is not None)


def bf16_rne(ref):
    """the one rounding a bf16 output carries: fp64 reference (exact in fp32) -> bf16 round to nearest even -> fp32."""
    r32 = ref.to(torch.float32)
    assert torch.equal(r32.double(), ref.double()), "the reference is not exact in fp32: the exactness bound is wrong"
    return r32.to(torch.bfloat16).to(torch.float32)


def _coords(mask, names, n):
    idx = mask.nonzero()[:n].tolist()
    return ", ".join("(" + " ".join(f"{k}={v}" for k, v in zip(names, i)) + ")" for i in idx)


def assert_bitexact(y, expect, names=("image", "channel", "w", "h"), what=""):
    """y equals expect element for element (-0 == +0); on a mismatch: how many differ and where (first coordinates, and which bands:
    wrap seam / boundary beams / last image), which usually names the bug."""
    y, expect = y.detach().float().cpu(), expect.detach().float().cpu()
    assert y.shape == expect.shape, f"{what}: shape {tuple(y.shape)} != {tuple(expect.shape)}"
    bad = ~(y == expect)
    n = int(bad.sum())
    if n == 0:
        return
    msg = [f"{what}: {n} of {y.numel()} elements differ; first at {_coords(bad, names, 6)}"]
    if y.dim() == 4 and names[0] == "image":
        B, _, W, H = y.shape
        for band, sl in (("column 0", bad[:, :, 0]), (f"column {W - 1}", bad[:, :, W - 1]), ("row 0", bad[..., 0]),
                         (f"row {H - 1}", bad[..., H - 1]), (f"image {B - 1}", bad[B - 1])):
            msg.append(f"{band}: {int(sl.sum())}")
        d = (y - expect)[bad]
        msg.append(f"max |diff| {float(d.abs().max()):.4g}")
    raise AssertionError("; ".join(msg))


def assert_banded_rel_l2(y, ref, tol, groups=None, what=""):
    """rel-L2 <= tol on the whole tensor AND separately on each band where a local error would hide in the whole-tensor norm:
    every (image, channel group) block (groups: the channels split into that many groups; a wrong image's GroupNorm statistics),
    output columns 0 and W-1 (wrap seam), rows 0 and H-1 (zero-padded beams) and the last image.  y, ref: (B, C, W, H)."""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    B, Cc, W, H = y.shape
    bands = [("whole", (slice(None),) * 4), (f"image {B - 1}", (B - 1,)), ("column 0", (slice(None), slice(None), 0)),
             (f"column {W - 1}", (slice(None), slice(None), W - 1)), ("row 0", (Ellipsis, 0)), (f"row {H - 1}", (Ellipsis, H - 1))]
    if groups:
        cg = Cc // groups
        bands += [(f"image {b} group {g}", (b, slice(g * cg, (g + 1) * cg))) for b in range(B) for g in range(groups)]
    worst = []
    for name, sl in bands:
        e = rel_l2(y[sl], ref[sl])
        if not e <= tol:
            worst.append(f"{name}: {e:.3g}")
    assert not worst, f"{what}: rel-L2 above {tol} on " + ", ".join(worst[:8]) + (f" (+{len(worst) - 8} more)" if len(worst) > 8 else "")


class RefCache:
    """fp64 references computed once per key (a shape runs under up to 9 routing flags with the same operands)."""

    def __init__(self, cap=64):
        self.d, self.cap = {}, cap

    def get(self, key, fn):
        if key not in self.d:
            if len(self.d) >= self.cap:
                self.d.pop(next(iter(self.d)))
            self.d[key] = fn()
        return self.d[key]


def silu_targets(values):
    """bf16 values h -> fp32 inputs beta with bf16(silu(beta)) == h for any silu accurate to 0.05 bf16 ulp: silu(beta) (fp64) lies
    within 0.05 ulp of h itself, so at least 0.45 ulp from a rounding midpoint.  (h >= -0.25; the branch of beta > -1.278.)"""
    out = []
    for h in values:
        h = float(h)
        b = 0.0 if h == 0 else (h if h > 1 else 1.0)
        for _ in range(100):                                # Newton on silu(b) = h
            s = 1.0 / (1.0 + np.exp(-b))
            f, df = b * s - h, s + b * s * (1 - s)
            b -= f / df
        b32 = float(np.float32(b))
        s = b32 / (1.0 + np.exp(-b32))
        ulp = 2.0 ** (np.floor(np.log2(abs(h))) - 7) if h != 0 else 2.0 ** -133
        assert abs(s - h) <= 0.05 * ulp, f"silu^-1({h}) not resolvable in fp32"
        out.append(b32)
    return torch.tensor(out, dtype=torch.float32)


# ---- selective-softmax operands (attention) -----------------------------------------------------------------------------------------
# Softmax is exact on operands built for it: if every query i gives one set S(i) of 2^j keys equal scores and every other key a
# score >= `gap` log2 units lower, the output is the mean of those keys' V rows (exact in bf16 for small integer V) on every route,
# in any tile order and whichever maximum stabilises the exponent.  Scores are in the kernels' log2 units: qh = bf16(q * log2(e) /
# sqrt(8)) against k.  Per head, dims 0..n-1 carry codes (query: alpha * the target's code, key: its own code, both +-1 and signed /
# permuted differently per (image, head)), dim 6 a tier (qh = 8) that lifts or sinks whole key tiles, dim 7 a fine tier (qh = 1/4).
# Every value is a bit pattern of per-token +-1 "bits" through one linear map, so the same q / k / v can also come out of
# GroupNorm -> to_q / to_k / to_v: x carries each bit and its negation in adjacent channels (every group: mean 0, variance 1).
QS_INFER = float(np.float32(1.4426950408889634) / np.sqrt(np.float32(8.0)))          # attention.hip / attn_q_scale, runtime.h (host, fp32)
QS_TRAIN = float(np.float32(0.35355339059327373) * np.float32(1.4426950408889634))   # train_attn.hip kScale * kLog2e (fp32)
R2_MARGINS, R3_MARGINS = (32, 48, 64, 88), (144, 160, 200)


def _prescaled(val, qs):
    """fp32 w with bf16(fp32(w * qs)) == val (what the kernels see after their own scaling and rounding)."""
    w = np.float32(val / qs)
    for _ in range(8):
        got = float(torch.tensor(float(np.float32(w) * np.float32(qs)), dtype=torch.float32).to(torch.bfloat16))
        if got == val:
            return float(w)
        w = np.nextafter(w, np.float32(np.inf) if got < val else np.float32(-np.inf), dtype=np.float32)
    raise AssertionError(f"no fp32 operand lands on {val} after * {qs} and bf16 rounding")


def _int_bits(v, nb):
    """integer values -> (nb, ...) +-1 bits and the affine map back: v = base + sum_b 2^(b-1) bit_b."""
    lo = int(v.min())
    u = (v - lo).long()
    assert int(u.max()) < 2 ** nb
    bits = torch.stack([((u >> b) & 1).float() * 2 - 1 for b in range(nb)])
    w = [2.0 ** (b - 1) for b in range(nb)]
    return bits, w, lo + sum(w)


def selective_operands(B, L, C, regime="R1", seed=0, alpha=16.0, gap=32, margin=None, fused=False):
    """q, k, v (B, L, C) fp32 with head h = channels 8h .. 8h+7, and qh = bf16(q * log2(e)/sqrt(8)) exactly as given.
    regime: R1 (every S(i) inside the first key tile), R2 / R3 (S(i) outside it, `margin` log2 units above its maximum: 30..90 = the
    fast path with P >> 1, >= 140 = the overflow fallback), stair (the maxima of the last <= 12 decoy tiles lie 7.75 and 8.25 log2 units
    above the running maximum in turn, just under and just over its threshold 8; S(i) in the last, ragged tile).  fused: C/2 bits per token (x has C
    channels), and the returned dict carries x, gamma, beta, wqkv, bqkv of a GroupNorm -> to_q / to_k / to_v that produces them."""
    g = torch.Generator().manual_seed(seed)
    H = C // 8
    F = C // 2 if fused else 32
    T = (L + 31) // 32
    if regime == "stair" and T < 2:
        regime = "R1"
    if regime in ("R2", "R3"):
        assert L > 32, "R2 / R3 need keys outside the first tile"
        if margin is None:
            margin = (R2_MARGINS if regime == "R2" else R3_MARGINS)[seed % (4 if regime == "R2" else 3)]
        assert margin % 8 == 0 and margin >= gap
    tier_bits = 8 if regime == "stair" else 1
    cap = {"R1": min(32, L), "R2": L - 32, "R3": L - 32, "stair": L - 32 * (T - 1)}[regime]
    e = cap.bit_length() - 1
    n = min(5, (F - tier_bits - 1) // 2, max(0, e - 1))       # j >= 1 where there is room: one selected key has dS = 0
    j = min(3, e - n)
    if regime in ("R2", "R3", "stair"):
        assert 2 ** n <= 32
    assert n >= 0 and j >= 0 and 2 * n + tier_bits <= F, (L, C, regime)
    Nc = 2 ** (n + j)
    # every tier sits below 0 so that the selected score is -8: a key past L read as zeros (score 0) would then win unless masked
    assert (n * alpha) % 8 == 0
    off = -int(n * alpha) // 8 - 1
    # ---- token roles and bits, per image ----
    bits = torch.randint(0, 2, (B, L, F), generator=g).float() * 2 - 1
    k6 = torch.zeros(B, L)
    k7 = torch.zeros(B, L)
    tb, kb = list(range(n)), list(range(n, 2 * n))
    tier0 = 2 * n
    for b in range(B):
        if regime == "R1":
            pos = torch.randperm(min(32, L), generator=g)[:Nc]
        elif regime == "stair":
            pos = 32 * (T - 1) + torch.randperm(cap, generator=g)[:Nc]
        else:
            pos = 32 + torch.randperm(L - 32, generator=g)[:Nc]
        coded = torch.zeros(L, dtype=torch.bool)
        coded[pos] = True
        codes = torch.arange(Nc) % (2 ** n)                     # 2^j keys per code
        for i, p in enumerate(pos.tolist()):
            for t in range(n):
                bits[b, p, kb[t]] = float(((int(codes[i]) >> t) & 1) * 2 - 1)
        if regime in ("R2", "R3", "stair"):                     # decoy tiles hold every code: their maximum is the tier's, for every query
            for t0 in range(0, 32 * (T - 1) if regime == "stair" else 32, 32):
                cov = torch.randperm(32, generator=g) % (2 ** n)
                for i in range(32):
                    for t in range(n):
                        bits[b, t0 + i, kb[t]] = float(((int(cov[i]) >> t) & 1) * 2 - 1)
        if regime == "stair":
            u = (torch.arange(T - 1) - max(0, T - 1 - 12)).clamp(min=0)
            umax = int(u.max())
            base = -(gap // 8) - (umax + 1) // 2 - 1
            lvl6 = base + u // 2 + u % 2
            lvl7 = u // 2 - u % 2
            k6[b, :32 * (T - 1)] = off + lvl6.repeat_interleave(32).float()
            k7[b, :32 * (T - 1)] = lvl7.repeat_interleave(32).float()
            k6[b, 32 * (T - 1):] = off + base                    # fillers of the last tile: the lowest tier
            k6[b, coded] = off
        else:
            drop = (margin if regime in ("R2", "R3") else gap) / 8
            k6[b] = torch.where(coded, float(off), off - drop)
    # tier bits (k6 and k7 as affine maps of bits)
    tier_map = []
    if regime == "stair":
        b6, w6, c6 = _int_bits(k6, 5)
        b7, w7, c7 = _int_bits(k7, 3)
        for t in range(5):
            bits[:, :, tier0 + t] = b6[t]
        for t in range(3):
            bits[:, :, tier0 + 5 + t] = b7[t]
        tier_map = [(6, [(tier0 + t, w6[t]) for t in range(5)], c6), (7, [(tier0 + 5 + t, w7[t]) for t in range(3)], c7)]
    else:
        lo = float(k6.min())
        bits[:, :, tier0] = torch.where(k6 == off, 1.0, -1.0)
        tier_map = [(6, [(tier0, (off - lo) / 2)], (off + lo) / 2), (7, [], 0.0)]
    pool = tb + list(range(tier0 + tier_bits, F))
    if len(pool) < 2:
        pool = list(range(F))
    # ---- per-head linear maps: rows of q (in qh units), k, v over the bits ----
    Wq, Wk, Wv = torch.zeros(3, C, F, dtype=torch.float64)
    bq, bk, bv = torch.zeros(3, C, dtype=torch.float64)
    for h in range(H):
        pq = torch.randperm(n, generator=g).tolist()
        pk = torch.randperm(n, generator=g).tolist()
        sq = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).tolist()
        sk = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).tolist()
        for d in range(n):
            Wq[8 * h + d, tb[pq[d]]] = alpha * sq[d]
            Wk[8 * h + d, kb[pk[d]]] = sk[d]
        for d in range(n, 6):                                   # dims no query reads: keys of one set differ there (dq != 0)
            Wk[8 * h + d, pool[int(torch.randint(0, len(pool), (1,), generator=g))]] = 1.0
        bq[8 * h + 6], bq[8 * h + 7] = 8.0, 0.25
        for d, terms, c0 in tier_map:
            for bit, w in terms:
                Wk[8 * h + d, bit] = w
            bk[8 * h + d] = c0
        for d in range(8):
            a, c = torch.randperm(len(pool), generator=g)[:2].tolist()
            s = float(torch.randint(0, 2, (1,), generator=g) * 2 - 1)
            Wv[8 * h + d, pool[a]], Wv[8 * h + d, pool[c]], bv[8 * h + d] = s, 2 * s, 4 * s
    bd = bits.double()
    qh, k, v = (bd @ W.T + bb for W, bb in ((Wq, bq), (Wk, bk), (Wv, bv)))
    out = dict(qh=qh.float(), k=k.float(), v=v.float(), n=n, j=j, regime=regime, margin=margin, gap=gap)
    for t in (out["qh"], out["k"], out["v"]):
        assert_on_grid(t, 0.25)
    out["q_infer"] = _from_qh(out["qh"], QS_INFER)
    out["q_train"] = _from_qh(out["qh"], QS_TRAIN)
    if fused:
        x = torch.zeros(B, L, C)
        x[..., 0::2], x[..., 1::2] = bits, -bits
        w = torch.zeros(3 * C, C)
        lut = {}
        for r in range(C):
            for m in range(F):
                if Wq[r, m] != 0:
                    val = float(Wq[r, m])
                    w[r, 2 * m] = lut.setdefault(val, _prescaled(val, QS_INFER))
        w[C:2 * C, 0::2], w[2 * C:, 0::2] = Wk.float(), Wv.float()
        bias = torch.cat([torch.tensor([_prescaled(float(t), QS_INFER) if t else 0.0 for t in bq]), bk.float(), bv.float()])
        eps = 1e-5
        out.update(x=x, wqkv=w, bqkv=bias.float(), eps=eps, groups=32 if C % 64 == 0 else C // 2,   # (an even count per group)
                   gamma=torch.full((C,), float(np.float32(np.sqrt(1 + eps)))), beta=torch.zeros(C))
    return out


def _from_qh(qh, qs):
    lut = {v: _prescaled(v, qs) for v in qh.unique().tolist()}
    return qh.clone().apply_(lambda t: lut[t])


def selective_reference(qh, k, v, j=None):
    """fp64 / exact analysis of selective operands (B, L, C): -> dict(out = mean of V over S(i) (B, L, C), count |S(i)|,
    smax = the selected score, gap = smax - best other key, margin = smax - maximum of the first key tile (B, H, L)).
    Scores are exact in fp32 (grid 1/16, < 2^24 units), so they are computed there, a few images at a time."""
    B, L, C = qh.shape
    H = C // 8
    chunk = max(1, 2 ** 24 // (H * L * L))
    res = {n: [] for n in ("out", "count", "smax", "gap", "margin")}
    for b0 in range(0, B, chunk):
        q4 = qh[b0:b0 + chunk].view(-1, L, H, 8).transpose(1, 2)
        k4 = k[b0:b0 + chunk].view(-1, L, H, 8).transpose(1, 2)
        v4 = v[b0:b0 + chunk].view(-1, L, H, 8).transpose(1, 2).double()
        s = q4 @ k4.transpose(-1, -2)
        smax = s.amax(-1, keepdim=True)
        sel = s == smax
        cnt = sel.sum(-1)
        other = torch.where(sel, torch.tensor(float("-inf")), s).amax(-1)
        res["out"].append(((sel.double() @ v4) / cnt[..., None].double()).transpose(1, 2).reshape(-1, L, C))
        res["count"].append(cnt)
        res["smax"].append(smax[..., 0].double())
        res["gap"].append((smax[..., 0] - other).double())
        res["margin"].append((smax[..., 0] - s[..., :min(32, L)].amax(-1)).double())
    r = {n: torch.cat(t) for n, t in res.items()}
    if j is not None:
        assert bool((r["count"] == 2 ** j).all()), "every S(i) must hold 2^j keys"
    return r


def bands_tokens(L):
    """token bands of a (B, L, C) attention output where a local error hides: first / last query tile, rows past the last full tile."""
    bands = [("first query tile", slice(0, min(32, L))), ("last query tile", slice(32 * ((L - 1) // 32), L))]
    if L % 32:
        bands.append(("rows past the last full tile", slice(L - L % 32, L)))
    return bands


def assert_banded_rel_l2_tokens(y, ref, tol, what=""):
    """rel-L2 <= tol on the whole (B, L, C) token-major tensor AND on each (image, head), the first / last query tile and the
    rows past the last full tile."""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    B, L, Cc = y.shape
    bands = [("whole", (slice(None),))] + [(name, (slice(None), sl)) for name, sl in bands_tokens(L)]
    bands += [(f"image {b} head {h}", (b, slice(None), slice(8 * h, 8 * h + 8))) for b in range(B) for h in range(Cc // 8)]
    worst = [f"{name}: {e:.3g}" for name, sl in bands for e in [rel_l2(y[sl], ref[sl])] if not e <= tol]
    assert not worst, f"{what}: rel-L2 above {tol} on " + ", ".join(worst[:8]) + (f" (+{len(worst) - 8} more)" if len(worst) > 8 else "")


# ---- GroupNorm operands whose statistics discriminate -------------------------------------------------------------------------------
# GroupNorm is exact on operands built for it.  Every (image, group) of cat[x0, x1] has its own location m = j s (|j| <= 3) and scale s
# (a power of two); every pixel of a channel takes one of two values, equally often, so the group mean and variance are known in closed
# form and the normalised value z = (x - mean) / sd is one of {+-1/5, +-7/5} (even channel count per group: the 3-4-5 form) or +-1
# (odd).  With gamma on a grid that carries the factor 5 and beta on the 1/4 grid, t = beta + gamma z is a 1/4-grid value per (channel,
# pixel value), the same for every image -- normalisation undoes m and s -- and only channels whose act(t) keeps >= 0.1 bf16 ulp from a
# rounding midpoint are kept.  A kernel's eps, rsqrt, fp32 variance and SiLU then cannot move bf16(act(t)): the map has one right answer.
GN_SCALES = (1.0, 2.0, 4.0, 8.0)        # s[b, g]: spread over a factor of 8
GN_TMAX = 4.0                           # |t| <= 4: every |act(t)| lies in [2^-4, 4] (silu(-4) = -0.0719, silu(-1.25) = -0.278, silu(-0.25) = -0.110)


def bf16_ulp(v):
    """bf16 unit in the last place at |v| (fp64 tensor, v != 0)."""
    return torch.exp2(torch.floor(torch.log2(v.abs())) - 7)


def bf16_midpoint_margin(v):
    """distance of v (fp64, != 0) from the nearest bf16 rounding midpoint, in bf16 ulps at v (0.5: v is a bf16 value)."""
    q = v.abs() / bf16_ulp(v)
    return (q - torch.floor(q) - 0.5).abs()


def _act64(t, silu):
    return t * torch.sigmoid(t) if silu else t


def gn_scales(B, groups, seed):
    """-> (j, s) (B, groups) fp64: location m = j s and scale s of every (image, group).  s differs between neighbouring images
    (b, (b + 1) % B) of a group and between neighbouring groups of an image, so (m, s) does."""
    assert B == 1 or (B - 1) % len(GN_SCALES) != 0, "the last image would share its scales with the first"
    g = torch.Generator().manual_seed(seed)
    r = int(torch.randint(0, len(GN_SCALES), (1,), generator=g))
    sidx = (torch.arange(B)[:, None] + torch.arange(groups)[None, :] + r) % len(GN_SCALES)
    s = torch.tensor(GN_SCALES, dtype=torch.float64)[sidx]
    j = torch.randint(-3, 4, (B, groups), generator=g).double()
    if B > 1:
        assert bool((s != s.roll(-1, 0)).all())
    assert bool((s[:, 1:] != s[:, :-1]).all())
    return j, s


def gn_operands(B, C0, C1, W, H, groups=32, seed=0, silu=True):
    """x0 (B, C0, W, H), x1 (B, C1, W, H) or None, gamma, beta (C0 + C1) fp32, and the exact GroupNorm(groups) (+ SiLU) map of cat[x0, x1].

    Even channel count per group (cpg): with u = s / 4, the first cpg / 2 channels of a group sit at m + 3u and the rest at m - 3u (or the
    other way round, seeded per (image, group)), each with spread +-4u: mean m, standard deviation exactly 5u, and the channels of one
    group -- and the two halves of a group -- have different means, so statistics per channel, over half a group or over two groups land
    elsewhere.  (First half / second half and not strictly alternating channels: alternating, half a group would have the group's own
    statistics, and `cpg per source` of two equal sources is half a group.)  Odd cpg: the plain two-valued form m +- s is enough (mean m,
    standard deviation s): no 3-4-5 split exists for an odd count, and a wrong image or a wrong group still changes s by a factor >= 2.
    The two values occur W H / 2 times each per channel in a seeded, irregular pattern over (w, h).

    -> dict(x0, x1, gamma, beta, expect = bf16(act(t)) as fp32, t (fp64, exact), mean, var (B, groups: closed forms), j, s, cpg,
    unit = the bf16 ulp of the smallest |expect| (every expect value is a multiple of it), amax = max |expect|)."""
    Cin, npx = C0 + C1, W * H
    assert Cin % groups == 0 and npx % 2 == 0
    cpg = Cin // groups
    even = cpg % 2 == 0
    g = torch.Generator().manual_seed(seed)
    j, s = gn_scales(B, groups, seed + 1)
    m = j * s
    u = s / 4 if even else s
    sd = 5 * u if even else u
    grp = torch.arange(Cin) // cpg
    if even:
        flip = (torch.randint(0, 2, (B, groups), generator=g) * 2 - 1).double()
        half = torch.where(torch.arange(Cin) % cpg < cpg // 2, 1.0, -1.0).double()
        off = 3 * half[None, :] * flip[:, grp]                                  # (B, Cin): +-3
    else:
        off = torch.zeros(B, Cin, dtype=torch.float64)
    r = torch.randint(0, 2, (B, Cin, npx // 2), generator=g, dtype=torch.int8)
    pm = torch.cat([r, 1 - r], -1)[..., torch.randperm(npx, generator=g)].double() * 2 - 1       # +-1, balanced per channel
    assert bool((pm.sum(-1) == 0).all())
    dev = off[..., None] + (4 if even else 1) * pm                              # (x - m) / u
    x = m[:, grp, None] + dev * u[:, grp, None]
    assert torch.equal(x.float().to(torch.bfloat16).double(), x), "values not exact in bf16"
    # ---- gamma, beta: per channel, redrawn until every value of t is safe ----
    zs = torch.tensor([-1.4, -0.2, 0.2, 1.4] if even else [-1.0, 1.0], dtype=torch.float64)
    gk = torch.tensor([-2.5, -1.25, 1.25, 2.5] if even else [-1.75, -1.25, -0.5, -0.25, 0.25, 0.5, 1.25, 1.75], dtype=torch.float64)
    sd_min = float(sd.min())
    shrink = sd_min / np.sqrt(sd_min * sd_min + 1e-5)                          # the largest effect of eps (<= 1e-5) on z
    gamma = torch.zeros(Cin, dtype=torch.float64)
    beta = torch.zeros(Cin, dtype=torch.float64)
    todo = torch.ones(Cin, dtype=torch.bool)
    for _ in range(200):
        n = int(todo.sum())
        if n == 0:
            break
        ga = gk[torch.randint(0, len(gk), (n,), generator=g)]
        be = torch.randint(-8, 9, (n,), generator=g).double() / 4
        t = be[:, None] + ga[:, None] * zs[None, :]
        t1 = be[:, None] + ga[:, None] * zs[None, :] * shrink
        ok = ((t != 0) & (t.abs() <= GN_TMAX)).all(-1)
        tt = torch.where(t == 0, torch.ones_like(t), t)
        a, a1 = _act64(tt, silu), _act64(torch.where(t == 0, tt, t1), silu)
        ok &= (bf16_midpoint_margin(a) >= 0.1).all(-1) & (bf16_midpoint_margin(a1) >= 0.1).all(-1)
        ok &= (a.float().to(torch.bfloat16) == a1.float().to(torch.bfloat16)).all(-1)
        idx = todo.nonzero()[:, 0][ok]
        gamma[idx], beta[idx] = ga[ok], be[ok]
        todo[idx] = False
    assert not bool(todo.any()), "no safe (gamma, beta) found for some channel"
    z = dev / (5 if even else 1)
    t = beta[None, :, None] + gamma[None, :, None] * z
    assert torch.equal(t * 4, (t * 4).round()) and bool((t != 0).all()) and float(t.abs().max()) <= GN_TMAX
    a = _act64(t, silu)
    assert float(bf16_midpoint_margin(a).min()) >= 0.1
    expect = a.float().to(torch.bfloat16).float()
    lo = float(expect.abs().min())
    assert lo >= 2.0 ** -4, "a value of the map below 2^-4: the exactness unit would shrink"
    unit = 2.0 ** (np.floor(np.log2(lo)) - 7)
    shape = (B, Cin, W, H)
    x = x.float().view(shape)
    return dict(x0=x[:, :C0].contiguous(), x1=x[:, C0:].contiguous() if C1 else None, gamma=gamma.float(), beta=beta.float(),
                expect=expect.view(shape), t=t.view(shape), mean=m, var=sd * sd, j=j, s=s, cpg=cpg, groups=groups, silu=silu,
                unit=unit, amax=float(expect.abs().max()))


def gn_bands(Cout, groups):
    """-> (nb, band of every output channel): nb = min(groups, Cout) bands of consecutive output channels."""
    nb = min(groups, Cout)
    return nb, torch.arange(Cout) * nb // Cout


def gn_block_weights(Cout, Cin, k, groups, seed, density=1.0):
    """weights (Cout, Cin, k, k) on the 2^-5 integer grid ({-4 .. 4} / 32), block-diagonal by group: the output channels form
    min(groups, Cout) bands, and band j reads the input groups g with g % bands == j only (Cout >= groups: input group j itself).
    A wrong output element then names its image and its input group(s)."""
    nb, band = gn_bands(Cout, groups)
    cpg = Cin // groups
    w = int_grid((Cout, Cin, k, k), seed, -4, 4, exp=-5, density=density)
    mask = (band[:, None] == (torch.arange(Cin) // cpg % nb)[None, :]).float()
    return w * mask[:, :, None, None]


def assert_bitexact_groups(y, expect, groups, what=""):
    """assert_bitexact for a conv with gn_block_weights: a mismatch names the (image, input group) bands that differ."""
    y, expect = y.detach().float().cpu(), expect.detach().float().cpu()
    assert y.shape == expect.shape, f"{what}: shape {tuple(y.shape)} != {tuple(expect.shape)}"
    bad = ~(y == expect)
    if not bool(bad.any()):
        return
    nb, band = gn_bands(y.shape[1], groups)
    per = torch.stack([bad[:, band == j].flatten(1).sum(1) for j in range(nb)], 1)          # (B, nb)
    where = [f"image {b} input group {j}" + (f" (mod {nb})" if nb < groups else "") + f": {int(per[b, j])}" for b, j in per.nonzero().tolist()]
    head = ", ".join(where[:8]) + (f" (+{len(where) - 8} more)" if len(where) > 8 else "")
    try:
        assert_bitexact(y, expect, what=what)
    except AssertionError as e:
        raise AssertionError(f"{e}; by (image, input group): {head}") from None


def assert_banded_rel_l2_groups(y, ref, tol, groups, what=""):
    """rel-L2 <= tol on every (image, GroupNorm group) block of a (B, C, W, H) tensor whose C channels form `groups` groups."""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    B, Cc = y.shape[:2]
    cg = Cc // groups
    worst = [f"image {b} group {g}: {e:.3g}" for b in range(B) for g in range(groups)
             for e in [rel_l2(y[b, g * cg:(g + 1) * cg], ref[b, g * cg:(g + 1) * cg])] if not e <= tol]
    assert not worst, f"{what}: rel-L2 above {tol} on " + ", ".join(worst[:8]) + (f" (+{len(worst) - 8} more)" if len(worst) > 8 else "")


def gn_shift_scale_tokens(o, seed):
    """selective_operands(fused=True) has every GroupNorm group of x at mean 0, variance 1.  -> x' = x s[b, g] + j[b, g] s[b, g]
    (gn_scales: powers of two, other (j, s) than the neighbouring image / group).  Normalisation undoes both, so q, k, v and the output
    are those of x.  The guards, asserted here: x' is exact in bf16 with exact fp32 channel sums; the kernels' folded weights
    W' = bf16(w32 a), a = gamma rsqrt(s^2 + eps) = (1 + d) / s with |d| <= eps / 2 + 8 fp32 ulps, stay on the bf16 values w32 / s; and the
    folded bias b' = b - sum_c w32[r, c] j (1 + d) misses its exact value by less than 0.1 bf16 ulp of the smallest q / k / v value of
    that row (rows that produce 0 have no weights)."""
    x = o["x"]
    B, L, C = x.shape
    G = o["groups"]
    cpg = C // G
    j, s = gn_scales(B, G, seed)
    grp = torch.arange(C) // cpg
    xs = (x.double() * s[:, None, grp] + (j * s)[:, None, grp])
    assert torch.equal(xs.float().to(torch.bfloat16).double(), xs) and float((xs * xs).sum(1).max()) < 2 ** 24
    xg = xs.view(B, L, G, cpg)
    assert torch.equal(xg.mean((1, 3)), j * s) and torch.equal((xg * xg).mean((1, 3)) - (j * s) ** 2, s * s)
    scale = torch.tensor([QS_INFER] * C + [1.0] * 2 * C, dtype=torch.float32)
    w32 = (o["wqkv"] * scale[:, None]).to(torch.bfloat16).float()
    dmax = o["eps"] / 2 + 8 * 2.0 ** -24
    for sv in GN_SCALES:
        for d in (-dmax, dmax):
            a = torch.tensor(float(np.float32((1 + d) / sv)))
            assert torch.equal((w32 * a).to(torch.bfloat16).float(), w32 / sv)
    err = 3 * w32.double().abs().sum(1) * (dmax + C * 2.0 ** -24)                      # (3C,)
    vals = torch.cat([o["qh"], o["k"], o["v"]], -1).double().abs().flatten(0, 1)         # (B L, 3C)
    lo = torch.where(vals == 0, torch.full_like(vals, float("inf")), vals).amin(0)
    assert bool((w32[(vals == 0).any(0)] == 0).all()), "a row that produces 0 carries weights"
    live = torch.isfinite(lo) & (err > 0)
    assert bool((err[live] <= 0.1 * bf16_ulp(lo[live])).all()), "the folded bias could move a q / k / v value"
    return xs.float()


# ---- placement: operands as the trainers place them ---------------------------------------------------------------------------------
# FlatParameters (tape.py) packs parameters and gradients end to end in flat buffers and TapeTrainer's ZeroArena packs split-K outputs at a 16-byte granule, so the
# other side of a view's last element is somebody else's live data.  `place` builds such a neighbourhood with known contents:
# [guard | t0 | guard | t1 | ... | guard] in ONE allocation, every view at the same offset modulo 16 bytes as the first (`lead`), every
# guard >= GUARD elements of one bit pattern.  Inputs sit between quiet NaNs (a stray load that is consumed -- also as x * 0 -- poisons the
# result); outputs sit between finite sentinels, their interior pre-filled with a second NaN pattern (an element never written shows;
# a cached block of an earlier call cannot hand it the right value); accumulating outputs carry the caller's pre-fill values.
# Caller-owned workspaces ("scratch": the *_workspace() sizes of train_disc.hip / train_meta.hip, the losses' partials) sit between the
# same finite sentinels and start from the unwritten-output pattern, but only their guards are checked: a workspace may stay partly
# unwritten (a route that needs no partials), and the low words of fp64 partials kept in an fp32 view can look like any fp32 NaN.
GUARD = 64
_PLACE_PATTERNS = {       # dtype: (integer view, NaN around inputs, NaN inside unwritten outputs, finite sentinel around outputs)
    torch.float32: (torch.int32, 0x7FC0A5A5, 0x7FC05A5A, 0xF5A5A5A5 - (1 << 32)),                         # sentinel = -4.2e32
    torch.bfloat16: (torch.int16, 0x7FE5, 0x7FDA, 0xF5A5 - (1 << 16)),
    torch.float64: (torch.int64, 0x7FF80000A5A5A5A5, 0x7FF800005A5A5A5A, 0xF5A5A5A5A5A5A5A5 - (1 << 64)),
}
PLACE_KINDS = ("in", "out", "acc", "scratch")


class Placement:
    """What `place` returns: buf[name] (or buf.views in order) are the contiguous views; the rest is assert_placement's record."""

    def __init__(self, flat, kind, names, views, spans, put):
        self.flat, self.kind, self.names, self.views, self.spans, self.put = flat, kind, names, views, spans, put

    def __getitem__(self, name):
        return self.views[self.names.index(name)] if isinstance(name, str) else self.views[name]

    def __iter__(self):
        return iter(self.views)

    def offset(self, name):
        """element offset of the view inside the allocation (offset % (16 / itemsize): its residue)"""
        return self.spans[self.names.index(name)][0]


def place(tensors, lead=GUARD, kind="in", device=None, dtype=None):
    """tensors: {name: tensor} (kind "in": the values; "acc": the pre-fill values of an accumulating output) or {name: shape} (kind
    "out": a non-accumulating output; "scratch": a caller-owned workspace of exactly that many elements).  lead: the first view's
    offset in elements (>= GUARD); lead % (16 bytes / itemsize) is the residue every view of the buffer gets (fp32: lead % 4).
    -> Placement."""
    assert kind in PLACE_KINDS, kind
    items = list(tensors.items())
    if dtype is None:
        dtype = next((t.dtype for _, t in items if torch.is_tensor(t)), torch.float32)
    if device is None:
        device = next((t.device for _, t in items if torch.is_tensor(t)), torch.device("cpu"))
    ityp, nan_in, nan_out, sentinel = _PLACE_PATTERNS[dtype]
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    assert lead >= GUARD, f"the leading guard needs {GUARD} elements"
    shapes = [tuple(t.shape) if torch.is_tensor(t) else tuple(int(v) for v in t) for _, t in items]
    spans, pos = [], lead
    for shp in shapes:
        n = int(np.prod(shp)) if len(shp) else 1
        spans.append((pos, n))
        pos += n + GUARD
        pos += (lead - pos) % per16                                  # the next view at the same residue
    total = pos                                                      # (the last guard is >= GUARD wide as well)
    bits = torch.full((total,), nan_in if kind == "in" else sentinel, dtype=ityp)
    for (start, n), (name, t) in zip(spans, items):
        if kind in ("out", "scratch"):
            bits[start:start + n] = nan_out
        else:
            assert torch.is_tensor(t) and t.dtype == dtype, f"{name}: kind {kind!r} needs a {dtype} tensor"
            bits[start:start + n] = t.detach().cpu().contiguous().view(-1).view(ityp)
    flat = bits.clone().to(device).view(dtype)                      # (`bits` stays as the record of what was put in)
    views = [flat[start:start + n].view(shp) for (start, n), shp in zip(spans, shapes)]
    return Placement(flat, kind, [n for n, _ in items], views, spans, bits)


def assert_placement(buf, what=""):
    """After the kernels ran: every guard of `buf` still holds its pattern bit for bit; kind "in": so does every interior (kernels do not
    write their inputs); kind "out": no interior element still holds the unwritten pattern, and none is any other NaN (the operands are
    finite: such a NaN was loaded from an input's guard); kind "scratch": the guards alone.  A failure names the operand, the side and
    the element offset relative to the operand's first element (negative: before it; >= its size: past it)."""
    ityp, nan_in, nan_out, sentinel = _PLACE_PATTERNS[buf.flat.dtype]
    now = buf.flat.detach().cpu().view(ityp)
    guard = torch.ones(now.numel(), dtype=torch.bool)
    for start, n in buf.spans:
        guard[start:start + n] = False
    bad = (guard & (now != (nan_in if buf.kind == "in" else sentinel))).nonzero().flatten().tolist()
    msgs = []
    for j in bad[:8]:
        # the nearer operand owns the complaint: past the end of the one before j, or before the start of the one behind j
        cands = []
        for name, (start, n) in zip(buf.names, buf.spans):
            if j >= start + n:
                cands.append((j - (start + n - 1), f"operand {name!r}: a store PAST the view, at element offset {j - start} (size {n})"))
            if j < start:
                cands.append((start - j, f"operand {name!r}: a store BEFORE the view, at element offset {j - start}"))
        msgs.append(min(cands)[1])
    if len(bad) > 8:
        msgs.append(f"(+{len(bad) - 8} more guard elements)")
    for name, (start, n) in zip(buf.names, buf.spans):
        if buf.kind == "scratch":                                    # a workspace: the guards above are all there is to ask
            continue
        cur = now[start:start + n]
        if buf.kind == "in":
            k = (cur != buf.put[start:start + n]).nonzero().flatten().tolist()
            if k:
                msgs.append(f"operand {name!r}: an INPUT was modified, {len(k)} elements, first at element offset {k[0]}")
        elif buf.kind == "out":
            k = (cur == nan_out).nonzero().flatten().tolist()
            if k:
                msgs.append(f"operand {name!r}: {len(k)} output elements NEVER WRITTEN, first at element offset {k[0]} (size {n})")
            vals = buf.flat[start:start + n].detach().cpu()
            k = (torch.isnan(vals) & (cur != nan_out)).nonzero().flatten().tolist()
            if k:
                msgs.append(f"operand {name!r}: {len(k)} output elements are NaN, first at element offset {k[0]}: finite operands give "
                            f"none, so a GUARD of an input was loaded and consumed")
        else:
            vals = buf.flat[start:start + n].detach().cpu()
            k = torch.isnan(vals).nonzero().flatten().tolist()
            if k:
                msgs.append(f"operand {name!r}: {len(k)} accumulated elements are NaN, first at element offset {k[0]}: finite operands "
                            f"give none, so a GUARD of an input was loaded and consumed")
    assert not msgs, f"{what}: " + "; ".join(msgs)


def flat_buffer_residues(names, shapes):
    """offset % 4 (in floats: the position inside a 16-byte granule) of every view FlatParameters._init_parameters makes for parameters
    packed end to end in the order `names`."""
    out, pos = set(), 0
    for n in names:
        out.add(pos % 4)
        pos += int(np.prod(shapes[n]))
    return out


def trainer_residues():
    """The residues the project's own trainers produce: VAEDecoderTrainer, VAETrainer (the shipped VAE), UNetTrainer (the full and the
    nuScenes configuration), from the shape tables and parameter orders those trainers use -- no GPU, no trainer object."""
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
    from rangeldm_amd.training import plan_parameter_order
    from rangeldm_amd.vae_training import decoder_param_names, encoder_param_names
    per = {}
    for preset in ("RangeLDM", "nuscenes"):
        vcfg, ucfg = PRESETS[preset]["vae"], PRESETS[preset]["unet"]
        vs = vae_param_shapes(vcfg)
        dec, enc = decoder_param_names(vcfg, vs), encoder_param_names(vcfg, vs)
        per[f"VAEDecoderTrainer/{preset}"] = flat_buffer_residues(dec, vs)
        per[f"VAETrainer/{preset}"] = flat_buffer_residues(enc + dec, vs)
        us = unet_param_shapes(ucfg)
        per[f"UNetTrainer/{preset}"] = flat_buffer_residues(plan_parameter_order(list(us), us)[0], us)
    return per


def flat_buffer_offsets(names, shapes):
    """name -> offset % 4 of its view, in the order `names` (what flat_buffer_residues collects into a set)."""
    out, pos = {}, 0
    for n in names:
        out[n] = pos % 4
        pos += int(np.prod(shapes[n]))
    return out


def discriminator_layouts():
    """name -> (trainable names in order, shapes) of every discriminator flat buffer the project builds or tests: the PatchGAN on the
    image (the reference's in_channels = 2, ndf = 64, n_layers = 3, and the small networks of the tests) and on the BEV volume
    (vae_training.py's disc_bev: in_channels = 2 gz planes, gz <= 16 and a channel count the 4x4 conv has an instance for: 2, 16, 32);
    the Meta-Kernel network at its default config (vae/configs/kitti360.yaml's) and at the configs of tests/disc_util.py and of the
    trainer tests (ndf = 16, one to three BatchNorm layers).  No GPU, no discriminator object."""
    from rangeldm_amd import discriminator as D
    from rangeldm_amd import metakernel as MK
    out = {}
    for tag, cfg in (("image", D.DiscriminatorConfig(2, 64, 3)), ("image/ndf16", D.DiscriminatorConfig(2, 16, 3)),
                     ("image/ndf16/n_layers1", D.DiscriminatorConfig(2, 16, 1)), ("disc_bev/gz1", D.DiscriminatorConfig(2, 64, 3)),
                     ("disc_bev/gz8", D.DiscriminatorConfig(16, 64, 3)), ("disc_bev/gz16", D.DiscriminatorConfig(32, 64, 3)),
                     ("disc_bev/gz16/ndf16", D.DiscriminatorConfig(32, 16, 3))):
        out["PatchDiscriminator/" + tag] = (D.trainable_names(cfg), D.param_shapes(cfg))
    for tag, cfg in (("default", MK.MetaKernelConfig()), ("ndf16", MK.MetaKernelConfig(2, 16, 3)), ("ndf16/n_layers2", MK.MetaKernelConfig(2, 16, 2)),
                     ("ndf16/n_layers1", MK.MetaKernelConfig(2, 16, 1))):
        out["MetaKernelDiscriminator/" + tag] = (MK.trainable_names(cfg), MK.param_shapes(cfg))
    return out


def discriminator_residues():
    """trainer_residues() for the two discriminators, which keep their parameters and gradients in FlatParameters' flat buffers as
    well and hand views of them to train_disc.hip / train_meta.hip (and to rldm_train_colsum): name -> set, over
    discriminator_layouts()."""
    return {k: flat_buffer_residues(names, shapes) for k, (names, shapes) in discriminator_layouts().items()}


# ---- the small models of the sampler and pipeline tests --------------------------------------------------------------------
def small_cfg(in_ch, out_ch):
    from rangeldm_amd.config import UNetConfig
    return UNetConfig(sample_size=(32, 8), in_channels=in_ch, out_channels=out_ch, block_out_channels=(32, 32, 64, 64))


def hip_unet(cfg, prefix):
    from rangeldm_amd.params import unet_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.unet import UNet2DModelHIP
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(synth_state_dict(unet_param_shapes(cfg), prefix=prefix))
    return m


_VAE = {}


def hip_vae():
    """One default-config VAE with synthetic weights, shared by every test that asks."""
    from rangeldm_amd.config import VAEConfig
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae import AutoencoderKLHIP
    if "m" not in _VAE:
        m = AutoencoderKLHIP(VAEConfig())
        m.load_state_dict(synth_state_dict(vae_param_shapes(VAEConfig()), prefix="vae."))
        _VAE["m"] = m
    return _VAE["m"]
