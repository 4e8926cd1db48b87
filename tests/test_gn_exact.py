"""GPU, bit-exact: every inference route that consumes GroupNorm statistics, on operands whose statistics differ per image and per group
(tests/hip_util.py gn_operands; proven on the CPU by tests/test_gn_operands.py).

Every (image, group) of cat[x0, x1] has its own location and power-of-two scale, the group mean and variance are exact closed forms, and
the normalised, activated map has one right bf16 value per element that no eps, rsqrt, fp32 variance or SiLU error of a kernel can move.
The conv behind it has weights on the 2^-5 integer grid that are block-diagonal by group (gn_block_weights), so its fp32 sums are exact
in any order and a wrong element names its image and input group.  A route that normalises image b with another image's statistics,
group g with a neighbour's, or counts the channels of a group per source, changes at least half of the elements of that band
(test_gn_operands.py), where the random-operand tests of test_hip_kernels.py stay inside their tolerance.  test_conv_exact.py covers the
same routes with gamma = 0: geometry, padding and epilogue, no statistics.
"""
import ctypes as C

import pytest
import torch

from oracle import ops
from rangeldm_amd import _lib
from rangeldm_amd._lib import Flag, Flag2
from tests.hip_util import (RefCache, amax, assert_bitexact, assert_bitexact_groups, assert_exact_bound, bf16_rne, gn_block_weights,
                            gn_operands, gn_shift_scale_tokens, hip_attention_qkv, hip_conv, hip_conv_stats, int_grid,
                            selective_operands, selective_reference)
from tests.test_hip_kernels import GN_CASES, conv_flags, regw_flags  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
B = 3                               # the last image is odd and differs from both neighbours
U = 2.0 ** -5                       # the weight / bias / time-embedding grid
_refs = RefCache(cap=48)


def conv_route(Bn, C0, C1, Cout, W, H, k=3, gn=True, silu=True, res=False, temb=False, stride=1):
    """the launches the plan of this conv consists of, as rldm_bench_conv names them: '[gn_apply+]<conv kernel>'."""
    d = _lib.ConvDescC()
    d.B, d.Cin0, d.Cin1, d.Win, d.Hin, d.Cout, d.ksize = Bn, C0, C1, W, H, Cout, k
    d.stride, d.pad_mode, d.upsample, d.gn, d.silu, d.eps = stride, 0, 0, int(gn), int(silu), 1e-5
    us, name = C.c_float(0), C.create_string_buffer(128)
    _lib.check(_lib.lib().rldm_bench_conv(C.byref(d), Cout if res else 0, int(temb), 0, 1, C.byref(us), name, 128,
                                          _lib.stream_ptr(torch.device("cuda"))), "rldm_bench_conv")
    return name.value.decode()


def _case(Bn, C0, C1, Cout, W, H, k, silu, seed, temb=False, res=False):
    """operands, block-diagonal weights thinned until the exactness bound holds, and the fp64 conv over the exact map (not yet rounded)."""
    o = gn_operands(Bn, C0, C1, W, H, 32, seed=seed, silu=silu)
    Cin = C0 + C1
    b = int_grid((Cout,), seed + 2, -64, 64, exp=-5)
    t = int_grid((Bn, Cout), seed + 3, -64, 64, exp=-5) if temb else None
    r = int_grid((Bn, Cout, W, H), seed + 4, -3, 3) if res else None
    density = 1.0
    while True:
        w = gn_block_weights(Cout, Cin, k, 32, seed + 1, density)
        try:
            # (an output's addends: |map| <= amax times its own weights, whose absolute sum bounds them however sparse they are)
            assert_exact_bound(o["unit"] * U, (1, o["amax"] * float(w.abs().sum((1, 2, 3)).max())), (1, amax(b)), (1, amax(t) if temb else 0),
                               (1, amax(r) if res else 0))
            break
        except AssertionError:
            assert density > 1 / 16
            density /= 2
    ref = ops.circ_conv2d(o["expect"].double(), w.double(), b.double(), 1, 1 if k == 3 else 0)
    if temb:
        ref = ref + t.double()[:, :, None, None]
    if res:
        ref = ref + r.double()
    return o, w, b, t, r, ref


# ---- the ResnetBlock conv1 fusion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0,C1,Cout,W,H", GN_CASES)
def test_conv_gn_silu_concat_temb_residual_exact(C0, C1, Cout, W, H, conv_flags):
    """GN(32) + SiLU over cat[x0, x1] -> conv3x3 + bias + temb[b] + res under every conv_flags routing: the in-staging folds of
    conv_igemm, conv_small and conv_stream (two channels per thread at 512 input channels: (256, 256, ...)), gn_apply in front of
    conv_small, groups that straddle the concat seam ((256, 128, ...): 12 channels per group) and 3 channels per group ((64, 32, ...))."""
    key = (C0, C1, Cout, W, H)

    def make():
        o, w, b, t, r, ref = _case(B, C0, C1, Cout, W, H, 3, True, 201, temb=True, res=True)
        return o, w, b, t, r, bf16_rne(ref)
    o, w, b, t, r, ref = _refs.get(("conv1",) + key, make)
    y = hip_conv(o["x0"], w, b, x1=o["x1"], gamma=o["gamma"], beta=o["beta"], silu=True, eps=1e-5, temb=t, res=r)
    assert_bitexact_groups(y, ref, 32, what=f"GN + SiLU conv {key} flags {conv_flags}")


OWN_IMAGE = [c for c in GN_CASES if c[3] * c[4] <= 64]        # images an image-owning conv_small tile takes: (32, 1), (32, 2), (16, 4)
_APPLY_LAUNCH = Flag.OWN_IMAGE_COPIES | Flag.NO_PERSISTENT


@pytest.mark.parametrize("C0,C1,Cout,W,H", OWN_IMAGE)
def test_conv_gn_apply_launch_exact(C0, C1, Cout, W, H):
    """norm.hip's gn_apply_kernel as a launch of its own in front of an image-owning conv_small: OWN_IMAGE_COPIES without the persistent
    launch (with it, conv_flags' "own-image-tiles" above, the same arithmetic runs as trunk.hip's gn_apply_phase)."""
    key = (C0, C1, Cout, W, H)

    def make():
        o, w, b, t, r, ref = _case(B, C0, C1, Cout, W, H, 3, True, 201, temb=True, res=True)
        return o, w, b, t, r, bf16_rne(ref)
    o, w, b, t, r, ref = _refs.get(("conv1",) + key, make)
    _lib.lib().rldm_debug_set_flags(_APPLY_LAUNCH)
    try:
        y = hip_conv(o["x0"], w, b, x1=o["x1"], gamma=o["gamma"], beta=o["beta"], silu=True, eps=1e-5, temb=t, res=r)
    finally:
        _lib.lib().rldm_debug_set_flags(0)
    assert_bitexact_groups(y, ref, 32, what=f"gn_apply + conv {key}")


# ---- conv_regw.hip: conv_c64 and the two fp32 output layers ------------------------------------------------------------------------------
C64_CASES = [(128, 16, True), (64, 32, False), (1024, 64, True)]     # (1024, 64): three images reach conv_regw's runs by default only there


@pytest.mark.parametrize("W,H,res", C64_CASES)
def test_conv_c64_register_weights_gn_exact(W, H, res, regw_flags):
    """64 -> 64, two channels per group, eps = 1e-6: conv_regw's runs (default at full resolution, REGW_CAP8 on small images) and
    conv_stream's per-tile instance (NO_REGW)."""
    def make():
        o, w, b, _, r, ref = _case(B, 64, 0, 64, W, H, 3, True, 211, res=res)
        return o, w, b, r, bf16_rne(ref)
    o, w, b, r, ref = _refs.get(("c64", W, H, res), make)
    y = hip_conv(o["x0"], w, b, gamma=o["gamma"], beta=o["beta"], silu=True, eps=1e-6, res=r)
    assert_bitexact_groups(y, ref, 32, what=f"c64 GN {B}x{W}x{H} res={res} flags {regw_flags}")


OUT_CASES = [(128, 16, 1), (64, 32, 4), (1024, 64, 2)]


@pytest.mark.parametrize("W,H,N", OUT_CASES)
@pytest.mark.parametrize("flags", [Flag2.FP32_OUT, Flag2.FP32_OUT | Flag2.REGW_CAP8, Flag2.FP32_OUT | Flag2.NO_REGW],
                         ids=["default", "runs-of-8-workgroups", "generic-kernel"])
def test_conv_out_fp32_nchw_gn_exact(W, H, N, flags):
    """the VAE decoder's output layer (64 -> N <= 4, fp32 NCHW): equal to the fp64 reference, no rounding.  Output channel o reads the
    input groups g with g % N == o."""
    def make():
        o, w, b, _, _, ref = _case(B, 64, 0, N, W, H, 3, True, 221)
        assert torch.equal(ref.float().double(), ref)
        return o, w, b, ref.float()
    o, w, b, ref = _refs.get(("out", W, H, N), make)
    _lib.lib().rldm_debug_set_flags2(flags)
    try:
        y = hip_conv(o["x0"], w, b, gamma=o["gamma"], beta=o["beta"], silu=True, eps=1e-6)
    finally:
        _lib.lib().rldm_debug_set_flags2(0)
    assert_bitexact_groups(y, ref, 32, what=f"conv_out GN {B}x{W}x{H} N={N} flags {flags!r}")


O4_CASES = [(256, 16, 4), (256, 16, 2), (1024, 8, 3)]


@pytest.mark.parametrize("W,H,N", O4_CASES)
@pytest.mark.parametrize("route", ["conv_o4", "generic"])
def test_unet_output_layer_gn_exact(W, H, N, route):
    """the UNet's conv_out (128 -> N <= 4, fp32 NCHW; conv_o4_kernel or the generic kernel): equal to the fp64 reference."""
    def make():
        o, w, b, _, _, ref = _case(B, 128, 0, N, W, H, 3, True, 231)
        assert torch.equal(ref.float().double(), ref)
        return o, w, b, ref.float()
    o, w, b, ref = _refs.get(("o4", W, H, N), make)
    _lib.lib().rldm_debug_set_flags2(Flag2.FP32_OUT)
    if route == "generic":
        _lib.lib().rldm_debug_set_flags(Flag.NO_CONV_SMALL | Flag.NO_STREAM_REGW)
    try:
        y = hip_conv(o["x0"], w, b, gamma=o["gamma"], beta=o["beta"], silu=True, eps=1e-5)
    finally:
        _lib.lib().rldm_debug_set_flags2(0)
        _lib.lib().rldm_debug_set_flags(0)
    assert_bitexact_groups(y, ref, 32, what=f"UNet conv_out GN {B}x{W}x{H} N={N} {route}")


# ---- pointwise, no SiLU ---------------------------------------------------------------------------------------------------------------
POINTWISE = [(256, 768, 32, 2, False), (128, 384, 128, 8, False), (256, 768, 64, 4, False), (512, 256, 16, 4, True), (128, 128, 16, 8, False)]


@pytest.mark.parametrize("Cc,N,W,H,res", POINTWISE)
def test_conv_pointwise_gn_exact(Cc, N, W, H, res):
    """conv_small.hip, taps == 1 (attention's group_norm -> Linear form): the affine folded into the staging, no SiLU, eps = 1e-6."""
    o, w, b, _, r, ref = _case(B, Cc, 0, N, W, H, 1, False, 241, res=res)
    y = hip_conv(o["x0"], w, b, gamma=o["gamma"], beta=o["beta"], silu=False, eps=1e-6, res=r)
    assert_bitexact_groups(y, bf16_rne(ref), 32, what=f"pointwise GN {(B, Cc, N, W, H, res)}")


# ---- which shapes reach which GroupNorm kernel ----------------------------------------------------------------------------------------
def test_gn_routes_reach_fold_apply_and_every_conv_family():
    """Which launch normalises, as rldm_bench_conv names the plan of each case.  gn_apply_kernel runs in front of conv_small exactly where
    a concatenated 3x3 input meets an image-owning tile (OWN_IMAGE: images of <= 64 pixels) and the persistent launch is off; with it
    on, those cases are phases of one persistent launch (no conv_* launch at all); every other case under every other routing folds the
    statistics in the conv's own staging.  The conv families are all there: conv_small, conv_stream, conv_igemm (generic), conv_regw.
    gn_fold_kernel folds an output's partials where an image has more than 32 pixel tiles (tiles hold <= 256 pixels): the 1024 x 64 and
    512 x 64 outputs of test_conv_statistics_exact and test_conv_c64_register_weights_statistics_exact; no entry point reports it."""
    lib = _lib.lib()

    def names(f1=0, f2=0):
        lib.rldm_debug_set_flags(f1)
        lib.rldm_debug_set_flags2(f2)
        try:
            return {c: conv_route(B, *c, res=True, temb=True) for c in GN_CASES}
        finally:
            lib.rldm_debug_set_flags(0)
            lib.rldm_debug_set_flags2(0)

    default, own, launch = names(), names(Flag.OWN_IMAGE_COPIES), names(_APPLY_LAUNCH)
    generic, anygrid = names(Flag.NO_CONV_SMALL | Flag.NO_STREAM_REGW), names(Flag.STREAM_ANY_GRID)
    assert {c for c, n in launch.items() if n.startswith("gn_apply+")} == set(OWN_IMAGE) and len(OWN_IMAGE) == 3, launch
    assert all("conv_small" in launch[c] for c in OWN_IMAGE), launch
    assert {c for c, n in own.items() if "conv_" not in n} == set(OWN_IMAGE), own
    assert not any(n.startswith("gn_apply+") for r in (default, own, generic, anygrid) for n in r.values())
    assert all(own[c] == default[c] for c in GN_CASES if c not in OWN_IMAGE)
    assert any("conv_small" in n for n in default.values()) and any("conv_stream" in n for n in default.values()), default
    assert any("conv_igemm" in n for n in default.values())
    assert any("conv_stream" in anygrid[c] and "conv_stream" not in default[c] for c in GN_CASES), anygrid
    assert all("conv_igemm" in n for n in generic.values()), generic
    # conv_regw's runs: by default only at full resolution, on small images under REGW_CAP8
    regw = {(W, H): conv_route(B, 64, 0, 64, W, H, res=res) for W, H, res in C64_CASES}
    assert [("conv_regw" in regw[(W, H)]) for W, H, _ in C64_CASES] == [False, False, True], regw
    lib.rldm_debug_set_flags2(Flag2.REGW_CAP8)
    try:
        assert all("conv_regw" in conv_route(B, 64, 0, 64, W, H, res=res) for W, H, res in C64_CASES)
    finally:
        lib.rldm_debug_set_flags2(0)
    assert all("conv_small" in conv_route(B, c[0], 0, c[1], c[2], c[3], k=1, silu=False, res=c[4]) for c in POINTWISE)
    assert all(W * H // 256 > 32 for W, H in ((1024, 64), (512, 64)))


# ---- the fused GroupNorm -> q / k / v attention launch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,L,Cc,regime", [(3, 100, 64, "R2"), (3, 64, 256, "R1"), (3, 1024, 128, "R3"), (3, 8, 32, "R1"), (16, 64, 256, "R2")])
def test_attention_qkv_shifted_scaled_groups_exact(Bn, L, Cc, regime):
    """selective_operands(fused=True) fixes every group at mean 0, variance 1; here x is scaled and shifted per (image, group) by powers
    of two.  Normalisation undoes both, so the output is the existing exact reference.  The guard that keeps the folded weights on their
    bf16 values and the folded bias within 0.1 ulp is asserted by gn_shift_scale_tokens (and on the CPU by test_gn_operands.py)."""
    def make():
        o = selective_operands(Bn, L, Cc, regime, seed=3, fused=True)
        ref = selective_reference(o["qh"], o["k"], o["v"], j=o["j"])
        return o, gn_shift_scale_tokens(o, seed=4), bf16_rne(ref["out"])
    o, xs, ref = _refs.get(("attn", Bn, L, Cc, regime), make)
    out = hip_attention_qkv(xs, o["gamma"], o["beta"], o["wqkv"], o["bqkv"], groups=o["groups"], eps=o["eps"])
    assert_bitexact(out, ref, ("image", "token", "channel"), f"attention_qkv shifted / scaled B{Bn} L{L} C{Cc} {regime}")


# ---- the statistics side outputs ------------------------------------------------------------------------------------------------------
def _stats_case(Bn, Cin, Cout, W, H, k, stride):
    """integer operands (x in [-3, 3], weights in {-1, 0, 1} thinned, integer bias): y is an integer, bf16(y) too, and the per-image sums
    of bf16(y) and bf16(y)^2 are exact fp32 sums in any order while they stay below 2^24."""
    x, b = int_grid((Bn, Cin, W, H), 251, -3, 3), int_grid((Cout,), 253, -4, 4)
    density = 0.5
    while True:
        w = int_grid((Cout, Cin, k, k), 252, -1, 1, density=density)
        assert_exact_bound(1.0, (Cin * k * k, amax(x) * amax(w)), (1, amax(b)))
        yq = bf16_rne(ops.circ_conv2d(x.double(), w.double(), b.double(), stride, 1 if k == 3 else 0)).double()
        s, q = yq.sum((2, 3)), (yq * yq).sum((2, 3))
        try:
            assert_exact_bound(1.0, (1, float(yq.abs().sum((2, 3)).max())))
            assert_exact_bound(1.0, (1, float(q.max())))
            return x, w, b, torch.stack([s, q], -1).float()
        except AssertionError:
            assert density > 1 / 64
            density /= 2


EPILOGUE_STATS = [(2, 128, 128, 64, 16, 3), (3, 64, 256, 32, 2, 3), (2, 32, 64, 16, 8, 1), (1, 128, 128, 256, 16, 3), (2, 256, 256, 64, 4, 3),
                  (16, 128, 256, 32, 2, 3), (2, 256, 256, 64, 4, 1), (16, 128, 128, 128, 8, 1), (2, 128, 128, 128, 8, 3),
                  (4, 256, 256, 32, 1, 3), (2, 256, 256, 32, 1, 1), (1, 64, 64, 1024, 64, 3), (16, 5, 128, 256, 16, 3)]


@pytest.mark.parametrize("Bn,Cin,Cout,W,H,k", EPILOGUE_STATS)
def test_conv_statistics_exact(Bn, Cin, Cout, W, H, k):
    """the (sum, sumsq) side output of the shapes of test_conv_epilogue_statistics, bit for bit ((1, 64, 64, 1024, 64): through gn_fold)."""
    x, w, b, ref = _stats_case(Bn, Cin, Cout, W, H, k, 1)
    assert_bitexact(hip_conv_stats(x, w, b), ref, ("image", "channel", "sum / sumsq"), f"statistics {(Bn, Cin, Cout, W, H, k)}")


@pytest.mark.parametrize("Bn,W,H", [(4, 512, 64), (2, 128, 16), (3, 64, 32)])
def test_conv_c64_register_weights_statistics_exact(Bn, W, H, regw_flags):
    """... of conv_regw's runs (one partial per workgroup, accumulated over the run; (4, 512, 64): through gn_fold)."""
    x, w, b, ref = _refs.get(("c64stats", Bn, W, H), lambda: _stats_case(Bn, 64, 64, W, H, 3, 1))
    assert_bitexact(hip_conv_stats(x, w, b), ref, ("image", "channel", "sum / sumsq"), f"c64 statistics {(Bn, W, H)} flags {regw_flags}")


@pytest.mark.parametrize("Bn,N,W,H", [(16, 256, 64, 4), (3, 64, 128, 2)])
def test_conv_stride2_statistics_exact(Bn, N, W, H):
    """... of the stride-2 down-sampler (conv_ds2_kernel: one partial per 32 x 1 output tile)."""
    x, w, b, ref = _stats_case(Bn, 256, N, W, H, 3, 2)
    assert_bitexact(hip_conv_stats(x, w, b, stride=2), ref, ("image", "channel", "sum / sumsq"), f"stride-2 statistics {(Bn, N, W, H)}")
