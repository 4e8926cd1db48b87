"""CPU: the GroupNorm operands of tests/test_gn_exact.py (tests/hip_util.py gn_operands / gn_block_weights) are what they claim --
closed-form statistics, the fp64 oracle's answer, its distance from every bf16 rounding midpoint -- and they discriminate: the map
computed with a neighbouring image's statistics, a neighbouring group's, or a channel count per group taken per source differs from the
right one in at least half of the affected elements."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops
from tests.hip_util import (GN_SCALES, RefCache, amax, assert_banded_rel_l2_groups, assert_bitexact_groups, assert_exact_bound, bf16_rne,
                            gn_block_weights, gn_operands)

# (B, C0, C1, W, H, silu): 2 / 3 (odd) / 4 / 6 / 8 / 12 (groups straddle the seam) / 16 channels per group, one and two sources
CASES = [(3, 64, 0, 16, 4, True), (3, 64, 32, 16, 8, True), (3, 128, 0, 16, 8, False), (3, 128, 64, 16, 4, True), (3, 128, 128, 16, 4, True),
         (3, 256, 128, 16, 8, True), (3, 256, 256, 32, 1, True), (2, 512, 0, 16, 4, False)]
_ops = RefCache(cap=len(CASES))


def bf16(t):
    return t.float().to(torch.bfloat16).float()


def _case(c):
    B, C0, C1, W, H, silu = c
    return _ops.get(c, lambda: gn_operands(B, C0, C1, W, H, 32, seed=11, silu=silu))


def _xc(o):
    return torch.cat([o["x0"], o["x1"]], 1).double() if o["x1"] is not None else o["x0"].double()


def _stats(xc, groups):
    xg = xc.reshape(xc.shape[0], groups, -1)
    mean = xg.mean(-1)
    return mean, (xg * xg).mean(-1) - mean * mean


def _apply(o, mean, var, eps=1e-5, cpg=None):
    """the GroupNorm (+ SiLU) map of the case with the given (B, groups) statistics -> bf16 values."""
    xc = _xc(o)
    grp = torch.arange(xc.shape[1]) // (cpg or o["cpg"])
    t = (xc - mean[:, grp, None, None]) / torch.sqrt(var[:, grp, None, None] + eps)
    t = t * o["gamma"].double()[None, :, None, None] + o["beta"].double()[None, :, None, None]
    return bf16(t * torch.sigmoid(t) if o["silu"] else t)


def _oracle(o, xc, gamma, beta, groups, eps):
    if o["silu"]:
        return ops.group_norm_silu(xc, gamma, beta, groups, eps)
    return F.group_norm(xc, groups, gamma, beta, eps)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c)))
def test_statistics_equal_the_closed_forms(c):
    o = _case(c)
    mean, var = _stats(_xc(o), 32)
    assert torch.equal(mean, o["mean"]) and torch.equal(var, o["var"])
    assert torch.equal(o["mean"], o["j"] * o["s"])
    u = o["s"] / 4 if o["cpg"] % 2 == 0 else o["s"]
    assert torch.equal(o["var"], (25 if o["cpg"] % 2 == 0 else 1) * u * u)
    assert set(o["s"].unique().tolist()) == set(GN_SCALES)
    B = c[0]
    ms = torch.stack([o["mean"], o["s"]], -1)
    assert bool((ms != ms.roll(-1, 0)).any(-1).all()) and bool((ms[:, 1:] != ms[:, :-1]).any(-1).all())
    # every value exact in bf16; two values per channel, equally often, no channel constant over a row or a column of pixels
    for x in (o["x0"], o["x1"]):
        if x is None:
            continue
        assert torch.equal(bf16(x), x)
        lo, hi = x.amin((2, 3), keepdim=True), x.amax((2, 3), keepdim=True)
        assert bool(((x == lo) | (x == hi)).all()) and bool(((x == hi).sum((2, 3)) * 2 == x.shape[2] * x.shape[3]).all())
    if o["cpg"] % 2 == 0:                        # the channels of a group have different means
        cm = _xc(o).mean((2, 3)).view(B, 32, o["cpg"])
        assert bool((cm[..., 0] != cm[..., -1]).all()) and bool((cm.mean(-1) == o["mean"]).all())


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c)))
def test_fp64_oracle_rounds_to_the_expected_map(c, eps):
    o = _case(c)
    ref = _oracle(o, _xc(o), o["gamma"].double(), o["beta"].double(), 32, eps)
    assert torch.equal(bf16(ref), o["expect"])
    # ... and stays clear of the rounding midpoints: the exact map by >= 0.1 ulp (asserted by the generator), the oracle's with eps too
    q = ref.abs() / torch.exp2(torch.floor(torch.log2(ref.abs())) - 7)
    assert float((q - q.floor() - 0.5).abs().min()) >= 0.09
    assert torch.equal(_apply(o, o["mean"], o["var"], eps), o["expect"])


@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c)))
def test_map_survives_kernel_arithmetic(c):
    """the affine scale a = gamma rsqrt(var + eps) off by +-8 fp32 ulps and the variance by 1e-5 relative: the same bf16 map."""
    o = _case(c)
    for ulps in (-8, 8):
        for dv in (-1e-5, 1e-5):
            oo = dict(o, gamma=o["gamma"].double() * (1 + ulps * 2.0 ** -24))
            assert torch.equal(_apply(oo, o["mean"], o["var"] * (1 + dv)), o["expect"]), (ulps, dv)


def _differs(o, wrong):
    """fraction of elements that differ, per (image, group) -> (B, groups)"""
    B = wrong.shape[0]
    d = (wrong != o["expect"]).view(B, 32, -1).double()
    return d.mean(-1)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wrong_image_statistics_change_the_map(c):
    o = _case(c)
    frac = _differs(o, _apply(o, o["mean"].roll(-1, 0), o["var"].roll(-1, 0)))          # image b reads image (b + 1) % B
    assert float(frac.min()) >= 0.5, frac


@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wrong_group_statistics_change_the_map(c):
    o = _case(c)
    frac = _differs(o, _apply(o, o["mean"].roll(-1, 1), o["var"].roll(-1, 1)))          # group g reads group g + 1
    assert float(frac[:, :-1].min()) >= 0.5, frac


@pytest.mark.parametrize("c", [c for c in CASES if c[2]], ids=lambda c: "x".join(map(str, c)))
def test_channel_count_per_source_changes_the_map(c):
    """GroupNorm(32) of each source on its own (C0 / 32 and C1 / 32 channels per group) instead of over the concatenation.
    Even count per group: every (image, group) differs in at least half of its elements.  Odd count (3 = 2 + 1 here): a group of the
    plain two-valued form has its own statistics in every channel, so only the wrong groups that straddle two right ones can differ;
    those do, in at least half of their elements."""
    o = _case(c)
    B, C0, C1 = c[0], c[1], c[2]
    g, b = o["gamma"].double(), o["beta"].double()
    wrong = bf16(torch.cat([_oracle(o, o["x0"].double(), g[:C0], b[:C0], 32, 1e-5),
                            _oracle(o, o["x1"].double(), g[C0:], b[C0:], 32, 1e-5)], 1))
    if o["cpg"] % 2 == 0:
        frac = _differs(o, wrong)
        assert float(frac.min()) >= 0.5, frac
    else:
        cw = C0 // 32
        straddle = [k for k in range(32) if (k * cw) // o["cpg"] != (k * cw + cw - 1) // o["cpg"]]
        assert straddle
        for k in straddle:
            d = (wrong[:, k * cw:(k + 1) * cw] != o["expect"][:, k * cw:(k + 1) * cw]).double().flatten(1).mean(1)
            assert float(d.min()) >= 0.5, (k, d)


@pytest.mark.parametrize("Cout,Cin,k", [(64, 64, 3), (256, 384, 3), (2, 64, 3), (4, 128, 3), (768, 256, 1), (192, 512, 3)])
def test_block_weights_localise(Cout, Cin, k):
    """band j of the output reads input group j (Cout >= 32) or the groups g % Cout == j: changing one input group changes that band only."""
    w = gn_block_weights(Cout, Cin, k, 32, seed=3)
    assert torch.equal(w * 32, (w * 32).round()) and float(w.abs().max()) <= 0.125
    nb = min(32, Cout)
    cpg = Cin // 32
    for gi in (0, 5, 31):
        rows = (w[:, gi * cpg:(gi + 1) * cpg].abs().sum((1, 2, 3)) != 0).nonzero()[:, 0]
        assert len(rows) and set((rows * nb // Cout).tolist()) == {gi % nb}


def test_conv_over_the_map_is_exact_and_names_the_group():
    """the caller's assert_exact_bound terms hold for the bf16 map, the fp64 conv over it is exact in fp32, and a statistics error in
    one (image, group) shows up in that band of the output and nowhere else."""
    o = gn_operands(3, 64, 64, 16, 4, 32, seed=5, silu=True)
    w = gn_block_weights(128, 128, 3, 32, seed=6)
    assert_exact_bound(o["unit"] * 2.0 ** -5, (o["cpg"] * 9, o["amax"] * amax(w)))
    ref = bf16_rne(ops.circ_conv2d(o["expect"].double(), w.double(), torch.zeros(128).double()))
    bad = o["expect"].clone()
    bad[1, 7 * 4:8 * 4] = _apply(o, o["mean"].roll(-1, 0), o["var"].roll(-1, 0))[1, 7 * 4:8 * 4]
    y = bf16_rne(ops.circ_conv2d(bad.double(), w.double(), torch.zeros(128).double()))
    with pytest.raises(AssertionError, match=r"by \(image, input group\): image 1 input group 7: \d+$"):
        assert_bitexact_groups(y, ref, 32, what="one group of one image")
    assert_bitexact_groups(ref, ref, 32)


def test_banded_groups_sees_one_group():
    ref = torch.randn(3, 64, 8, 4, generator=torch.Generator().manual_seed(0))
    assert_banded_rel_l2_groups(ref * (1 + 1e-5), ref, 1e-4, 32)
    z = ref.clone()
    z[2, 10:12] *= 1.01
    with pytest.raises(AssertionError, match="image 2 group 5"):
        assert_banded_rel_l2_groups(z, ref, 1e-4, 32)


@pytest.mark.parametrize("B,L,C,regime", [(3, 100, 64, "R2"), (3, 64, 256, "R1"), (3, 8, 32, "R1"), (2, 48, 16, "R1")])
def test_shifted_scaled_tokens_normalise_to_the_same_map(B, L, C, regime):
    """gn_shift_scale_tokens asserts its own guards (folded weights on their bf16 values, folded bias within 0.1 ulp); the fp64 oracle
    normalises x' to the map of x."""
    from tests.hip_util import gn_shift_scale_tokens, selective_operands
    o = selective_operands(B, L, C, regime, seed=3, fused=True)
    xs = gn_shift_scale_tokens(o, seed=4)
    assert not torch.equal(xs, o["x"])

    def norm(x):
        x = x.double().transpose(1, 2).unsqueeze(-1)
        return F.group_norm(x, o["groups"], o["gamma"].double(), o["beta"].double(), o["eps"])
    assert float((norm(xs) - norm(o["x"])).abs().max()) < 1e-5
