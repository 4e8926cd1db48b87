"""CPU: the exact-operand helpers of tests/hip_util.py (the bit-exact GPU tests are only as good as these)."""
import pytest
import torch

from oracle import ops
from tests.hip_util import (RefCache, assert_banded_rel_l2, assert_bitexact, assert_exact_bound, assert_on_grid, bf16_rne, int_grid,
                            silu_targets)


def test_int_grid_is_bf16_exact_seeded_and_in_range():
    a = int_grid((64, 33, 5), seed=3, lo=-4, hi=4, exp=-5)
    assert_on_grid(a, 2.0 ** -5)
    assert torch.equal(a, int_grid((64, 33, 5), seed=3, lo=-4, hi=4, exp=-5))
    assert not torch.equal(a, int_grid((64, 33, 5), seed=4, lo=-4, hi=4, exp=-5))
    q = a * 32
    assert float(q.min()) == -4 and float(q.max()) == 4 and len(q.unique()) == 9
    big = int_grid((4096,), seed=1, lo=-256, hi=256)
    assert_on_grid(big, 1.0)
    sparse = int_grid((10000,), seed=2, lo=1, hi=3, density=0.25)
    assert 0.2 < float((sparse != 0).float().mean()) < 0.3
    with pytest.raises(AssertionError):
        int_grid((4,), seed=0, lo=-257, hi=3)
    with pytest.raises(AssertionError):
        assert_on_grid(torch.tensor([1.0, 257.0]), 1.0)            # 9 significant bits
    with pytest.raises(AssertionError):
        assert_on_grid(torch.tensor([0.5]), 1.0)


def test_exact_bound_accepts_in_range_and_rejects_over_range():
    u = 2.0 ** -5
    assert assert_exact_bound(u, (512 * 9, 3 * 4 * u), (1, 2.0)) < 2 ** 24
    with pytest.raises(AssertionError):
        assert_exact_bound(u, (2 ** 21, 3 * 4 * u))                  # 12 * 2^21 units
    with pytest.raises(AssertionError):
        assert_exact_bound(1.0, (1, 2.0 ** 24))
    # ... and the bound is what it claims: at 2^24 units fp32 stops being exact
    assert float(torch.tensor(2.0 ** 24, dtype=torch.float32) + 1) == 2.0 ** 24


def test_conv_on_grid_is_exact_in_fp32_in_any_order():
    """the premise: an fp32 conv of grid operands inside the bound equals the fp64 one exactly (torch's own fp32 CPU conv here)."""
    x = int_grid((2, 64, 16, 4), seed=1)
    w = int_grid((32, 64, 3, 3), seed=2, lo=-4, hi=4, exp=-5)
    b = int_grid((32,), seed=3, lo=-64, hi=64, exp=-5)
    assert_exact_bound(2.0 ** -5, (64 * 9, 3 * 4 * 2.0 ** -5), (1, 2.0))
    r64 = ops.circ_conv2d(x.double(), w.double(), b.double())
    assert torch.equal(ops.circ_conv2d(x, w, b).double(), r64)
    assert torch.equal(bf16_rne(r64), r64.to(torch.bfloat16).float())


def test_bf16_rne_rounds_ties_to_even_and_refuses_inexact_references():
    r = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    assert bf16_rne(r).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]
    with pytest.raises(AssertionError):
        bf16_rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


def test_assert_bitexact_reports_count_and_coordinates():
    a = torch.zeros(2, 3, 8, 4)
    assert_bitexact(a, -a)                                           # -0 == +0
    b = a.clone()
    b[1, 2, 7, 0] = 2 ** -20
    b[0, 1, 0, 3] = 1.0
    with pytest.raises(AssertionError) as e:
        assert_bitexact(b, a, what="case")
    s = str(e.value)
    assert "2 of 192 elements differ" in s and "(image=0 channel=1 w=0 h=3)" in s and "(image=1 channel=2 w=7 h=0)" in s
    assert "column 0: 1" in s and "column 7: 1" in s and "image 1: 1" in s
    b[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_bitexact(b, b)                                        # NaN never matches


def test_banded_rel_l2_sees_a_local_error_the_whole_tensor_forgives():
    ref = torch.randn(4, 64, 32, 32, generator=torch.Generator().manual_seed(0))
    y = ref * (1 + 1e-3)
    assert_banded_rel_l2(y, ref, 4e-3, groups=32)
    for sl in ((slice(None), slice(None), 0), (Ellipsis, 31), (3,), (1, slice(10, 12))):
        z = ref.clone()
        z[sl] *= 1.015
        assert float((z - ref).norm() / ref.norm()) < 4e-3 or sl == (3,)
        with pytest.raises(AssertionError):
            assert_banded_rel_l2(z, ref, 4e-3, groups=32)


def test_silu_targets_round_to_their_bf16_values():
    h = torch.tensor([k / 8 for k in range(-2, 17)], dtype=torch.float32)
    beta = silu_targets(h)
    assert torch.equal(torch.nn.functional.silu(beta.double()).to(torch.bfloat16).float(), h)
    assert torch.equal(torch.nn.functional.silu(beta).to(torch.bfloat16).float(), h)


def test_ref_cache_computes_once_and_stays_bounded():
    c, calls = RefCache(cap=2), []
    for k in (1, 1, 2, 1, 3, 3, 1):
        c.get(k, lambda k=k: calls.append(k) or k)
    assert calls == [1, 2, 3, 1] and len(c.d) <= 2
