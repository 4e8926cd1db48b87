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
