"""GPU, bit-exact: every inference conv route on integer-grid operands (tests/hip_util.py: int_grid / assert_exact_bound).

Activations / residuals are integers in [-3, 3], weights in {-4 .. 4} * 2^-5, bias / time embedding on the 2^-5 grid: every product is
exact in fp32 and so is every sum (in any order: MFMA chains, k-groups, split K), which each test asserts from its own operands.  A
route then has one right answer, the fp64 reference of oracle/ops.py rounded once to the output type: bf16 round to nearest even for
the bf16 tensors, nothing for the fp32 output layers.  A lost tap, a stale halo, a wrong seam or a skipped epilogue term changes
elements that a whole-tensor relative-L2 gate (test_hip_kernels.py) forgives.

GroupNorm's rsqrt and SiLU's exp are not exact: the GroupNorm routes run with gamma = 0, where the normalised map is act(beta), one
value per channel, chosen so that its bf16 rounding cannot depend on the kernel's exp (hip_util.silu_targets).  That pins zero padding
AFTER normalisation (beams -1 and H read 0, not act(beta)), the wrap seam of the normalised map, the concatenation seam, the
per-channel beta indexing and the epilogue; the random-operand tests of test_hip_kernels.py check the statistics, band by band.
"""
import pytest
import torch

from oracle import ops
from rangeldm_amd._lib import Flag, Flag2
from tests.hip_util import (RefCache, amax, assert_bitexact, assert_exact_bound, bf16_rne, hip_conv, int_grid, silu_targets)
from tests.test_hip_kernels import CONV_CASES, GN_CASES, conv_flags, regw_flags  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
U = 2.0 ** -5                       # the weight / bias grid; activations are integers, so every addend is a multiple of U
_refs = RefCache(cap=64)


def _x(shape, seed):
    return int_grid(shape, seed, -3, 3)


def _w(shape, seed):
    return int_grid(shape, seed, -4, 4, exp=-5)


def _b(shape, seed):
    return int_grid(shape, seed, -64, 64, exp=-5)


def _conv64(x, w, b, stride=1, pad_mode=0, up=False):
    x, w, b = x.double(), w.double(), b.double()
    if up:
        return ops.upsample_conv(x, w, b)
    if stride == 2 and pad_mode == 1:
        return ops.downsample_vae(x, w, b)
    return ops.circ_conv2d(x, w, b, stride, 1 if w.shape[2] == 3 else 0)


# ---- A: no GroupNorm ------------------------------------------------------------------------------------------------------------------
def _geometry_case(case):
    B, Cin, Cout, W, H, k, s, pm, up = case
    x, w, b = _x((B, Cin, W, H), 101), _w((Cout, Cin, k, k), 102), _b((Cout,), 103)
    assert_exact_bound(U, (Cin * k * k, amax(x) * amax(w)), (1, amax(b)))
    return x, w, b, bf16_rne(_conv64(x, w, b, s, pm, up))


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_geometry_exact(case, conv_flags):
    """every CONV_CASES shape under every routing: stride 2, VAE end pad, nearest x2 (folded and sub-pixel), conv_c16, conv_ds2, H = 1,
    N = 2 / 4 masking."""
    B, Cin, Cout, W, H, k, s, pm, up = case
    x, w, b, ref = _refs.get(("geometry", case), lambda: _geometry_case(case))
    y = hip_conv(x, w, b, stride=s, pad_mode=pm, upsample=up)
    assert_bitexact(y, ref, what=f"conv {case} flags {conv_flags}")


@pytest.mark.parametrize("B,W,H,res", [(2, 128, 16, False), (2, 1024, 64, True), (3, 64, 32, True), (4, 512, 64, False)])
def test_conv_c64_register_weights_exact(B, W, H, res, regw_flags):
    """conv_regw.hip's 64 -> 64 conv without GroupNorm (+ the identity residual), under every regw_flags routing."""
    x, w, b = _x((B, 64, W, H), 111), _w((64, 64, 3, 3), 112), _b((64,), 113)
    r = _x((B, 64, W, H), 114) if res else None
    assert_exact_bound(U, (576, amax(x) * amax(w)), (1, amax(b)), (1, amax(r) if res else 0))

    def ref():
        out = _conv64(x, w, b)
        return bf16_rne(out + r.double() if res else out)

    y = hip_conv(x, w, b, res=r)
    assert_bitexact(y, _refs.get(("c64", B, W, H, res), ref), what=f"c64 {B}x{W}x{H} res={res} flags {regw_flags}")


@pytest.mark.parametrize("B,C,N,W,H", [(2, 256, 256, 32, 2), (4, 256, 256, 32, 1), (16, 128, 128, 128, 8), (2, 128, 384, 128, 8)])
def test_conv_pointwise_small_route_exact(B, C, N, W, H):
    """conv_small.hip, taps == 1, identity residual in the epilogue (attention output projections), and a q/k/v-width 1x1 without."""
    x, w, b = _x((B, C, W, H), 121), _w((N, C, 1, 1), 122), _b((N,), 123)
    r = _x((B, N, W, H), 124) if N == C else None
    assert_exact_bound(U, (C, amax(x) * amax(w)), (1, amax(b)), (1, amax(r) if r is not None else 0))
    y = hip_conv(x, w, b, res=r)
    ref = _conv64(x, w, b)
    assert_bitexact(y, bf16_rne(ref + r.double() if r is not None else ref), what=f"pointwise {B}x{C}x{N}x{W}x{H}")


def _epilogue_case(C0, C1, Cout, W, H):
    B, Cin = 2, C0 + C1
    x0, x1 = _x((B, C0, W, H), 131), _x((B, C1, W, H), 132)
    w, b = _w((Cout, Cin, 3, 3), 133), _b((Cout,), 134)
    temb, res = _b((B, Cout), 135), _x((B, Cout, W, H), 136)
    assert_exact_bound(U, (Cin * 9, amax(x0, x1) * amax(w)), (1, amax(b)), (1, amax(temb)), (1, amax(res)))
    ref = _conv64(torch.cat([x0, x1], 1), w, b) + temb.double()[:, :, None, None] + res.double()
    return x0, x1, w, b, temb, res, bf16_rne(ref)


@pytest.mark.parametrize("C0,C1,Cout,W,H", GN_CASES)
def test_conv_concat_temb_residual_exact(C0, C1, Cout, W, H, conv_flags):
    """two sources (x1), bias, time embedding and residual on the routes that take them without GroupNorm."""
    x0, x1, w, b, temb, res, ref = _refs.get(("epilogue", C0, C1, Cout, W, H), lambda: _epilogue_case(C0, C1, Cout, W, H))
    y = hip_conv(x0, w, b, x1=x1, temb=temb, res=res)
    assert_bitexact(y, ref, what=f"concat + temb + res {(C0, C1, Cout, W, H)} flags {conv_flags}")


# ---- B1: GroupNorm routes with gamma = 0 ----------------------------------------------------------------------------------------------
H_GRID = [k / 8 for k in range(-2, 17)]          # act(beta) values: 2^-3 grid, |h| <= 2 (exact in bf16)
HU = 2.0 ** -3


def _gn_beta(Cin, seed, silu):
    """per-channel beta whose act(beta) is a 2^-3 grid value; -> (beta, act(beta) as exact values)."""
    idx = torch.randint(0, len(H_GRID), (Cin,), generator=torch.Generator().manual_seed(seed))
    h = torch.tensor(H_GRID, dtype=torch.float32)[idx]
    return (silu_targets(h) if silu else h.clone()), h


def _gn0_ref(h, B, W, H, w, b, temb=None, res=None, stride=1):
    """conv over the constant-per-channel normalised map (zero padded in H AFTER normalisation, wrapped in W)."""
    hm = h.double()[None, :, None, None].expand(B, -1, W, H).contiguous()
    out = ops.circ_conv2d(hm, w.double(), b.double(), stride, 1 if w.shape[2] == 3 else 0)
    if temb is not None:
        out = out + temb.double()[:, :, None, None]
    if res is not None:
        out = out + res.double()
    return out


def _gn0_case(C0, C1, Cout, W, H):
    B, Cin = 2, C0 + C1
    x0, x1 = _x((B, C0, W, H), 141) * 0.5 + 0.25, _x((B, C1, W, H), 142)
    w, b = _w((Cout, Cin, 3, 3), 143), _b((Cout,), 144)
    beta, h = _gn_beta(Cin, 145, True)
    temb, res = _b((B, Cout), 146), _x((B, Cout, W, H), 147)
    assert_exact_bound(HU * U, (Cin * 9, max(abs(v) for v in H_GRID) * amax(w)), (1, amax(b)), (1, amax(temb)), (1, amax(res)))
    return x0, x1, w, b, beta, temb, res, bf16_rne(_gn0_ref(h, B, W, H, w, b, temb, res))


@pytest.mark.parametrize("C0,C1,Cout,W,H", GN_CASES)
def test_conv_gn_silu_concat_temb_residual_gamma0_exact(C0, C1, Cout, W, H, conv_flags):
    """the ResnetBlock conv1 fusion with gamma = 0: GN(32) + SiLU over cat[x0, x1] is silu(beta) per channel."""
    x0, x1, w, b, beta, temb, res, ref = _refs.get(("gn0", C0, C1, Cout, W, H), lambda: _gn0_case(C0, C1, Cout, W, H))
    y = hip_conv(x0, w, b, x1=x1, gamma=torch.zeros(C0 + C1), beta=beta, silu=True, eps=1e-5, temb=temb, res=res)
    assert_bitexact(y, ref, what=f"GN(gamma=0) + SiLU conv {(C0, C1, Cout, W, H)} flags {conv_flags}")


@pytest.mark.parametrize("B,W,H,res", [(4, 512, 64, True), (2, 128, 16, False), (3, 64, 32, True), (1, 256, 8, False)])
def test_conv_c64_register_weights_gamma0_exact(B, W, H, res, regw_flags):
    x = _x((B, 64, W, H), 151)
    w, b = _w((64, 64, 3, 3), 152), _b((64,), 153)
    beta, h = _gn_beta(64, 154, True)
    r = _x((B, 64, W, H), 155) if res else None
    assert_exact_bound(HU * U, (576, 2 * amax(w)), (1, amax(b)), (1, amax(r) if res else 0))
    y = hip_conv(x, w, b, gamma=torch.zeros(64), beta=beta, silu=True, eps=1e-6, res=r)
    ref = _refs.get(("c64gn0", B, W, H, res), lambda: bf16_rne(_gn0_ref(h, B, W, H, w, b, res=r)))
    assert_bitexact(y, ref, what=f"c64 GN(gamma=0) {B}x{W}x{H} res={res} flags {regw_flags}")


@pytest.mark.parametrize("B,C,N,W,H,res", [(2, 256, 768, 32, 2, False), (16, 128, 384, 128, 8, False), (4, 256, 768, 64, 4, False),
                                           (3, 512, 256, 16, 4, True)])
def test_conv_pointwise_gn_gamma0_exact(B, C, N, W, H, res):
    """conv_small.hip, taps == 1, GroupNorm affine folded into the staging (no SiLU): the map is beta itself."""
    x, w, b = _x((B, C, W, H), 161), _w((N, C, 1, 1), 162), _b((N,), 163)
    beta, h = _gn_beta(C, 164, False)
    r = _x((B, N, W, H), 165) if res else None
    assert_exact_bound(HU * U, (C, 2 * amax(w)), (1, amax(b)), (1, amax(r) if res else 0))
    y = hip_conv(x, w, b, gamma=torch.zeros(C), beta=beta, silu=False, eps=1e-6, res=r)
    assert_bitexact(y, bf16_rne(_gn0_ref(h, B, W, H, w, b, res=r)), what=f"pointwise GN(gamma=0) {(B, C, N, W, H, res)}")


@pytest.mark.parametrize("B,W,H,N", [(4, 512, 64, 2), (2, 128, 16, 1), (3, 64, 32, 4)])
@pytest.mark.parametrize("flags", [Flag2.FP32_OUT, Flag2.FP32_OUT | Flag2.REGW_CAP8, Flag2.FP32_OUT | Flag2.NO_REGW],
                         ids=["default", "runs-of-8-workgroups", "generic-kernel"])
def test_conv_out_fp32_nchw_gamma0_exact(B, W, H, N, flags):
    """the VAE decoder's output layer (fp32 NCHW, no output rounding): equal to the fp64 reference."""
    from rangeldm_amd import _lib
    x, w, b = _x((B, 64, W, H), 171), _w((N, 64, 3, 3), 172), _b((N,), 173)
    beta, h = _gn_beta(64, 174, True)
    assert_exact_bound(HU * U, (576, 2 * amax(w)), (1, amax(b)))
    _lib.lib().rldm_debug_set_flags2(flags)
    try:
        y = hip_conv(x, w, b, gamma=torch.zeros(64), beta=beta, silu=True, eps=1e-6)
    finally:
        _lib.lib().rldm_debug_set_flags2(0)
    assert_bitexact(y, _gn0_ref(h, B, W, H, w, b).float(), what=f"conv_out {B}x{W}x{H} N={N} flags {flags}")


@pytest.mark.parametrize("B,W,H,N", [(16, 256, 16, 4), (3, 256, 16, 2), (2, 1024, 8, 4)])
@pytest.mark.parametrize("route", ["conv_o4", "generic"])
def test_unet_output_layer_gamma0_exact(B, W, H, N, route):
    """the UNet's conv_out (conv_regw.hip's conv_o4_kernel, or the generic kernel): fp32 NCHW, equal to the fp64 reference."""
    from rangeldm_amd import _lib
    x, w, b = _x((B, 128, W, H), 181), _w((N, 128, 3, 3), 182), _b((N,), 183)
    beta, h = _gn_beta(128, 184, True)
    assert_exact_bound(HU * U, (1152, 2 * amax(w)), (1, amax(b)))
    _lib.lib().rldm_debug_set_flags2(Flag2.FP32_OUT)
    if route == "generic":
        _lib.lib().rldm_debug_set_flags(Flag.NO_CONV_SMALL | Flag.NO_STREAM_REGW)
    try:
        y = hip_conv(x, w, b, gamma=torch.zeros(128), beta=beta, silu=True, eps=1e-5)
    finally:
        _lib.lib().rldm_debug_set_flags2(0)
        _lib.lib().rldm_debug_set_flags(0)
    assert_bitexact(y, _gn0_ref(h, B, W, H, w, b).float(), what=f"UNet conv_out {B}x{W}x{H} N={N} {route}")


@pytest.mark.parametrize("B,W,H,N", [(2, 128, 16, 1), (3, 64, 32, 4)])
def test_conv_out_fp32_nchw_exact(B, W, H, N):
    """... and without GroupNorm: the fp32 output of the plain conv equals the fp64 reference."""
    from rangeldm_amd import _lib
    x, w, b = _x((B, 64, W, H), 191), _w((N, 64, 3, 3), 192), _b((N,), 193)
    assert_exact_bound(U, (576, amax(x) * amax(w)), (1, amax(b)))
    _lib.lib().rldm_debug_set_flags2(Flag2.FP32_OUT)
    try:
        y = hip_conv(x, w, b)
    finally:
        _lib.lib().rldm_debug_set_flags2(0)
    assert_bitexact(y, _conv64(x, w, b).float(), what=f"fp32 conv_out {B}x{W}x{H} N={N}")
