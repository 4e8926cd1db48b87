"""Frechet distance over dumped activations on the device (rangeldm_amd/csrc/frechet.hip; rangeldm_amd.metrics.gram_f64 /
singular_values / frechet_distance; `evaluate frd`).

Gram product.  On integer-valued operands with |v| <= 64 every product and every partial sum is an integer below 2^53, so
whatever order the fp64 MFMA adds in, the result is exact: it must equal numpy's integer product bit for bit.  The shapes
cover one instruction, every edge (n1, n2 not multiples of 16, d not a multiple of 4), the K tail of the 32-wide LDS stage
and several 64 x 64 tiles each way.

Singular values.  One-sided Jacobi and LAPACK are both backward stable, so they differ by c * 2^-52 * sigma_max with a
modest c that grows with the rotations a column takes (sweeps x columns).  c is not measured on a device: it is the worst
case of tests/test_frechet_host.py: jacobi_host, the numpy restatement of the same scheme (same pairs, same order of
rotations, same skip rule; only the order inside a reduction differs), against np.linalg.svd over sv_cases().
test_constants_of_the_numpy_restatement in that file reproduces the figures:

    random_33x20 6.9   random_20x33 5.8   odd_columns_31x7 4.2   zero_column 2.8   equal_columns 1.3
    rank5_in_40x40 17.3 (17 sweeps)   orthogonal 0.75 (numpy's own error; ours is exact)   one_by_one 0
    random_300x257 132.8 (12 sweeps)

SV_C_RESTATED is the worst of them; the tests allow 8 x that.  Every test prints its own figure before it asserts.

Frechet distance.  Differences are relative to Tr C1 + Tr C2 (tests/test_frechet_host.py: frechet_comparisons lists every
comparison).  By the same restatement: fixture cases against frechet_distance_host 0 / 7.8 / 18.2 / 1.9, rank 40 in
150 x 90 39.4, swapped arguments 1.0, identical sets against 0 97.5 (22 sweeps), a shifted copy against |v|^2 95.5
(x 2^-52).  FRD_C_RESTATED is the worst; the tests allow 8 x that.  Against the reference's own values the bound is
test_frechet_host.REF_RTOL (sqrtm's noise on a singular product).
"""
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd import metrics as M
from test_frechet_host import (FRD_C_RESTATED, REF_RTOL, SV_C_RESTATED, frechet_cases, frechet_comparisons, property_inputs,
                                sv_cases, trace_scale)
from test_generation_metrics import _run_evaluate

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SV_TOL = 8 * SV_C_RESTATED * EPS
FRD_TOL = 8 * FRD_C_RESTATED * EPS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- Gram product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16, 4), (17, 33, 5), (1, 1, 1), (48, 31, 259), (130, 65, 1024)], ids=str)
def test_gram_is_exact_on_integer_operands(shape):
    n1, n2, d = shape
    rng = np.random.default_rng(n1 * 1000 + n2)
    a = rng.integers(-64, 65, (n1, d))
    b = rng.integers(-64, 65, (n2, d))
    got = M.gram_f64(_dev(a.astype(np.float64)), _dev(b.astype(np.float64)))
    assert got.dtype == torch.float64 and tuple(got.shape) == (n1, n2)
    want = (a @ b.T).astype(np.float64)
    wrong = int((got.cpu().numpy() != want).sum())
    print(f"{shape}: {wrong} of {n1 * n2} entries differ")
    assert wrong == 0


def test_gram_entry_depends_on_its_two_rows_alone():
    rng = np.random.default_rng(7)
    a, b = _dev(rng.normal(size=(21, 77))), _dev(rng.normal(size=(70, 77)))
    whole = M.gram_f64(a, b)
    assert torch.equal(M.gram_f64(a[3:9], b), whole[3:9])
    assert torch.equal(M.gram_f64(a, b[5:69]), whole[:, 5:69])
    assert torch.equal(M.gram_f64(a, b), whole)
    ref = a.cpu().numpy() @ b.cpu().numpy().T
    # a 77-term dot product in any order is within 77 u sum |a b| of the exact one (u = 2^-53); two of them, device and numpy
    bound = 77 * EPS * (np.abs(a.cpu().numpy()) @ np.abs(b.cpu().numpy()).T)
    assert np.all(np.abs(whole.cpu().numpy() - ref) <= bound)


# ---- singular values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sv_cases(), ids=lambda c: c[0])
def test_singular_values_against_numpy(case):
    name, m = case
    got, sweeps = M.singular_values(_dev(m), return_sweeps=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (min(m.shape),)
    got = got.cpu().numpy()
    want = np.linalg.svd(m, compute_uv=False)
    c = float(np.abs(got - want).max() / (EPS * want[0]))
    print(f"{name}: {sweeps} sweeps; worst |device - numpy| = {c:.2f} x 2^-52 sigma_max")
    assert np.all(np.diff(got) <= 0) and np.all(got >= 0)
    assert 1 <= sweeps < _lib.RLDM_FRECHET_MAX_SWEEPS
    if name == "orthogonal":
        assert sweeps == 1 and np.array_equal(got, 4.0 * np.arange(16.0, 0.0, -1.0))      # no rotation: the norms, exactly
    if name == "zero_column":
        assert got[-1] == 0.0
    if name == "one_by_one":
        assert sweeps == 1 and got[0] == 3.5
    assert np.abs(got - want).max() <= SV_TOL * want[0]


def test_singular_values_orientation_and_repeat():
    rng = np.random.default_rng(12)
    m = _dev(rng.normal(size=(26, 9)))
    a, sa = M.singular_values(m, return_sweeps=True)
    b, sb = M.singular_values(m.t(), return_sweeps=True)       # the same columns after the orientation swap
    assert torch.equal(a, b) and sa == sb
    assert torch.equal(M.singular_values(m), a)
    assert torch.equal(M.singular_values(m.float().double()), M.singular_values(m.float()))
    with pytest.raises(ValueError, match="NaN or inf"):
        bad = m.clone()
        bad[3, 4] = float("inf")
        M.singular_values(bad)


def test_sweep_cap_is_reported_not_waited_for():
    m = _dev(np.random.default_rng(13).normal(size=(26, 9)))
    with pytest.raises(M.FrechetConvergenceError, match="sweep 1"):       # one sweep of a random matrix rotates: the cap
        M.singular_values(m, max_sweeps=1)
    sv, sweeps = M.singular_values(m, return_sweeps=True)                   # and the next call is untouched by it
    assert 1 < sweeps < _lib.RLDM_FRECHET_MAX_SWEEPS and torch.equal(sv, M.singular_values(m))


# ---- Frechet distance -----------------------------------------------------------------------------------------------------
def _report(what, got, want, scale):
    c = abs(got - want) / (EPS * scale)
    print(f"{what}: device {got!r} against {want!r}: difference = {c:.2f} x 2^-52 (Tr C1 + Tr C2)")
    return abs(got - want)


@pytest.mark.parametrize("case", frechet_cases(), ids=lambda c: c[0])
def test_frechet_distance_on_the_fixture_cases(case):
    name, x, y, ref = case
    terms = M.frechet_distance(_dev(x), _dev(y), return_terms=True)
    got, scale = terms["frd"], trace_scale(x, y)
    assert set(terms) == {"frd", "mean_sq", "tr1", "tr2", "tr_sqrt", "sweeps"}
    assert got == terms["mean_sq"] + terms["tr1"] + terms["tr2"] - 2.0 * terms["tr_sqrt"]
    assert got == M.frechet_distance(_dev(x), _dev(y))
    assert 1 <= terms["sweeps"] < _lib.RLDM_FRECHET_MAX_SWEEPS
    # sums of n d <= 4096 squares in two different orders (blocked / pairwise: a few dozen roundings deep at the most)
    assert abs(terms["tr1"] + terms["tr2"] - scale) <= 64 * EPS * scale
    d_host = _report(f"{name} (host)", got, M.frechet_distance_host(x, y), scale)
    d_ref = _report(f"{name} (reference)", got, ref, scale)
    assert d_host <= FRD_TOL * scale
    assert d_ref <= REF_RTOL * scale
    if name.startswith("same"):
        assert abs(got) <= FRD_TOL * scale


def test_frechet_distance_properties():
    worst = 0.0
    for name, got, want, scale in frechet_comparisons(lambda x, y: M.frechet_distance(_dev(x), _dev(y))):
        worst = max(worst, _report(name, got, want, scale) / scale)
    assert worst <= FRD_TOL
    x, y, _ = property_inputs()
    assert M.frechet_distance(_dev(x), _dev(y)) == M.frechet_distance(_dev(x), _dev(y))       # two calls: bit-identical


def test_frechet_distance_dtypes_and_nan():
    rng = np.random.default_rng(22)
    x32, y32 = _dev(rng.normal(size=(20, 24)).astype(np.float32)), _dev(rng.normal(size=(17, 24)).astype(np.float32))
    want = M.frechet_distance(x32.double(), y32.double(), return_terms=True)
    assert M.frechet_distance(x32, y32, return_terms=True) == want
    assert M.frechet_distance(x32, y32.double(), return_terms=True) == want
    assert want["sweeps"] >= 1
    bad = y32.clone()
    bad[5, 7] = float("nan")
    with pytest.raises(ValueError, match="NaN or inf"):
        M.frechet_distance(x32, bad)
    assert _lib.lib().rldm_frechet_last_sweeps() == 0        # refused before the Jacobi loop: not one sweep was run
    with pytest.raises(ValueError, match="NaN or inf"):
        M.frechet_distance(bad, x32)
    assert M.frechet_distance(x32, y32, return_terms=True) == want                 # and the next call is what it was


# ---- the driver -----------------------------------------------------------------------------------------------------------
def test_evaluate_frd_one_process_and_two_ranks(tmp_path):
    rng = np.random.default_rng(31)
    total, count = 4 * 8 * 8, 16
    folders = []
    for name, shift in (("a", 0.0), ("b", 0.4)):
        d = tmp_path / name
        d.mkdir()
        for i in range(8):
            np.save(str(d / f"{i:03d}.npy"), rng.normal(shift, 1.0, (4, 8, 8)).astype(np.float32))
        folders.append(str(d))
    out = tmp_path / "frd.json"
    args = ["frd", *folders, "--total", str(total), "--count", str(count)]
    one = _run_evaluate(1, args + ["--json", str(out)], timeout=300)
    res = json.loads(one)
    assert set(res) == {"task", "frd", "mean_sq", "tr1", "tr2", "tr_sqrt", "sweeps", "n1", "n2", "dims"}
    assert (res["task"], res["n1"], res["n2"], res["dims"]) == ("frd", 8, 8, count)
    assert out.read_text() == one + "\n"
    idx = M.frd_indices(total, count)
    x, y = (M.load_activations(f, idx, total=total) for f in folders)
    want = M.frechet_distance(x, y, return_terms=True)
    assert res["frd"] == want["frd"] and {k: res[k] for k in want} == want
    # (only now, after the first launches succeeded) two ranks: rank 0 alone computes, the output is byte-identical
    assert _run_evaluate(2, args, timeout=300) == one
