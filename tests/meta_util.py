"""The integer-valued operands of the Meta-Kernel's exact layer tests (tests/test_metakernel_gpu.py).  The golden file and the
sequences on it are tests/disc_util.py's (`META`)."""
import numpy as np
import torch

from rangeldm_amd import metakernel as MK

# ---- integer-valued operands of one layer ------------------------------------------------------------------------------------------
# Everything the kernels round to bf16 is an integer of at most 8 bits, and every sum is exact in fp32 in any order:
#   r in {0, 4, 8} (100 outside H); cos_azi, sin_azi in {0, +-1/4}, cos_inc, sin_inc in {0, +-1}: pe is integer-valued, |pe| <= 33
#   W1 has one entry of +-5 per row and b1 is a multiple of 5: pre is a multiple of 5, |pre| <= 170, and LeakyReLU's 0.2 (fp32:
#   0.2 (1 + 1.5e-8); fp64: 0.2 (1 + 5.6e-17)) times a multiple of 5 rounds to the integer pre / 5 in either precision
#   W2 has one entry of +-1 per row, b2 in [-2, 2]: |m| <= 172;  x in {-1, 0, 1};  coov in {-1, 0, 1}
#   dy in {0, +-5}: G = dy coov and dm = G x are multiples of 5, so the masked dh is integer-valued as well
# exact_layer_case() checks the bf16 grid and the fp32 bound on the values it made, not on worst cases.
_EXACT = {}


def exact_layer_case(B, W, H, Cc, N, stride, seed=0):
    """-> dict of float32 torch tensors (x NHWC, r, tables (4, 16), w1, b1, w2, b2, coov (N, 16 C), bias, dy NHWC) and `ref`:
    layer_host's fp64 result with dr_next given."""
    key = (B, W, H, Cc, N, stride, seed)
    if key in _EXACT:
        return _EXACT[key]
    g = torch.Generator().manual_seed(4000 + seed + 7 * Cc + N)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()      # noqa: E731
    Wo, Ho = (W - 2) // stride + 1, (H - 2) // stride + 1
    c = dict(x=ri(-1, 1, (B, W, H, Cc)), r=4 * ri(0, 2, (B, W, H)),
             tables=torch.cat([ri(-1, 1, (2, 16)) / 4, ri(-1, 1, (2, 16))]),
             b1=5 * ri(-1, 1, (Cc,)), b2=ri(-2, 2, (Cc,)), coov=ri(-1, 1, (N, 16 * Cc)), bias=ri(-3, 3, (N,)),
             dy=5 * ri(-1, 1, (B, Wo, Ho, N)), dr_next=ri(-3, 3, (B, Wo, Ho)))
    w1 = torch.zeros(Cc, 3)
    w1[torch.arange(Cc), torch.randint(0, 3, (Cc,), generator=g)] = 5 * (ri(0, 1, (Cc,)) * 2 - 1)
    w2 = torch.zeros(Cc, Cc)
    w2[torch.arange(Cc), torch.randint(0, Cc, (Cc,), generator=g)] = ri(0, 1, (Cc,)) * 2 - 1
    c["w1"], c["w2"] = w1, w2
    n = {k: v.numpy() for k, v in c.items()}
    ref = MK.layer_host(n["x"], n["r"], n["tables"], n["w1"], n["b1"], n["w2"], n["b2"], n["coov"], n["bias"], stride, dy=n["dy"],
                        dr_next=n["dr_next"])
    # the grid and the bounds, on the values themselves
    mm = MK.mlp_host(ref["pe"], n["w1"], n["b1"], n["w2"], n["b2"])
    cv = MK.modconv_host(n["x"], ref["src"], ref["m"], n["coov"], n["bias"], n["dy"])
    src = ref["src"]
    xp = np.where((src >= 0)[:, None], n["x"].reshape(-1, Cc)[np.maximum(src, 0)], 0.0)
    P = ref["m"] * xp
    dpre = (cv["dm"] @ n["w2"].astype(np.float64)) * np.where(ref["pe"] @ n["w1"].T.astype(np.float64) + n["b1"] > 0, 1.0, 0.2)

    def bf16_exact(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).float()
        return bool(torch.equal(t.to(torch.bfloat16).float().double(), torch.from_numpy(np.ascontiguousarray(a)).double()))
    for name, a in (("h", mm["h"]), ("m x", P), ("dy", n["dy"]), ("dm", cv["dm"]), ("W2", n["w2"]), ("coov", n["coov"])):
        assert bf16_exact(a), f"{name} is not exact in bf16"
    a_ = np.abs
    rows = src.size
    sums = dict(y=a_(P).reshape(-1, 16 * Cc) @ np.ones(16 * Cc) + 3, G=a_(n["dy"]).reshape(-1, N) @ a_(n["coov"]),
                dcoov=a_(n["dy"]).reshape(-1, N).T @ a_(P).reshape(-1, 16 * Cc), dw2=a_(cv["dm"]).T @ a_(mm["h"]),
                dh=a_(cv["dm"]) @ a_(n["w2"]), dw1=a_(dpre).T @ a_(ref["pe"]), dpe=a_(dpre) @ a_(n["w1"]),
                db=rows * max(a_(cv["dm"]).max(), a_(dpre).max()))
    sums["dx"] = 16 * sums["G"].max() * a_(ref["m"]).max()          # at most sixteen rows read a pixel
    sums["dr"] = 65 * sums["dpe"].max() + 3                         # sixteen rows as a tap (three terms each), sixteen as the centre
    for name, s in sums.items():
        assert float(np.max(s)) < 2 ** 22, f"{name}: sums of up to {float(np.max(s)):.3g} quarter-units are not exact in fp32"
    c["ref"] = ref
    _EXACT[key] = c
    return c
