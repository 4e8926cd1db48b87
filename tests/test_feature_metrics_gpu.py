"""Kernel distance and precision / recall / density / coverage on the device (rangeldm_amd/csrc/feature_metrics.hip;
rangeldm_amd.metrics.feature_scan / knn_radii_sq / prdc / kernel_distance; `evaluate features`).

Exact cases.  On integer-valued features with entries in -L .. L every product, every partial sum and (s_a + s_b) - 2 g are
integers far below 2^53 (the largest squared distance of the cases is 15 870), so whatever order the fp64 MFMA adds in, every
squared distance is exact: each output of feature_scan and the four scores of prdc must equal the int64 brute force
((a[:, None] - b[None]) ** 2).sum(-1) bit for bit.  Three generated rows equal real rows and one real row duplicates its
neighbour, and the small alphabets make squared distances that EQUAL a radius common (the test counts them, on numpy alone,
before it looks at the device), so the strict `<` and the ties are exercised.  For the kernel, d = 64 and entries in
-2 .. 2 make t = g / 64 + 1 = m / 64 with |m| <= 320 and t^3 = m^3 / 2^18 exact, and sums of a few thousand of those too.

Tiles per chunk.  A column chunk is one tile of 64 columns for every n_b <= 1024, so only a larger b makes a workgroup take
a second trip through its tile loop: reload the row's k + 1 smallest values, keep the threshold, and go on counting and
summing.  The `..._with_several_tiles_per_chunk` tests run at n_b = 1025 .. 2049 (two and three tiles per chunk; a last chunk
of 1, 76, 129 and 128 columns) with k up to FEATURE_K_CAP = 16, the longest list a row keeps: exactly on integer features
(test_feature_metrics_host.LARGE_EXACT_CASES, whose host test asserts that rows really have their nearest columns in several
tiles of one chunk), for the kernel sums, for the fold over gram_f64's values on real data, and for row independence.

Real-valued cases (test_feature_metrics_host.real_case).  A d-term dot product in any order is within
d 2^-53 sum |a b| <= d 2^-54 (s_i + s_j) of the exact one, so device and numpy squared distances differ by at most

    D2_BOUND(i, j) = 4 (d + 2) 2^-52 (s_i + s_j)

(two products' errors twice over, two norms', and the roundings of the sum and the difference).  Sorted values inherit the
largest bound of their row.  A count may differ from numpy's only through a pair whose d2 lies within that bound (plus the
radius' own) of the radius it is compared with: each test first asserts, on numpy alone, that its case has no such pair,
and then requires the counts and the four scores to be EQUAL.  A kernel term t^3, t = g / d + 1, is held to
3 t^2 |dg| / d + 4 2^-52 |t^3| with |dg| <= d 2^-52 sum |a| |b|, summed over the row.  Each test prints its worst ratio to
its bound before it asserts.
"""
import functools
import json
import math

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M
from test_feature_metrics_host import (LARGE_EXACT_CASES, LARGE_REAL_SHAPE, REAL_SHAPES, exact_inputs, large_exact_case,
                                       nearest_column_spread, real_case, real_inputs)
from test_generation_metrics import _run_evaluate

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
EXACT_CASES = [(17, 33, 4, 1, 2), (65, 63, 33, 5, 3), (130, 64, 259, 5, 8), (64, 129, 32, 5, 2)]      # (N, M, d, k, L)
OUTPUTS = ("kmin_sq", "count_a", "count_b", "min_sq", "poly_sum")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same_scan(got, want):
    """Every output of two FeatureScans of device tensors is bit-identical (and the same ones are absent)."""
    for name in OUTPUTS:
        g, w = getattr(got, name), getattr(want, name)
        assert (g is None) == (w is None), name
        assert g is None or torch.equal(g, w), name


# ---- exact on integer-valued features -------------------------------------------------------------------------------------
def _exact_inputs(case):
    return exact_inputs(EXACT_CASES[case], 100 + case)


def _brute(a, b):
    return ((a[:, None, :].astype(np.int64) - b[None, :, :].astype(np.int64)) ** 2).sum(-1)


@pytest.mark.parametrize("case", range(len(EXACT_CASES)), ids=[str(c) for c in EXACT_CASES])
def test_scan_and_prdc_are_exact_on_integer_features(case):
    real, fake, k = _exact_inputs(case)
    _assert_scan_and_prdc_are_the_brute_force(EXACT_CASES[case], real, fake, k, _brute(real, real), _brute(fake, fake), _brute(real, fake))


@pytest.mark.parametrize("case", range(len(LARGE_EXACT_CASES)), ids=[str(c) for c in LARGE_EXACT_CASES])
def test_scan_and_prdc_are_exact_with_several_tiles_per_chunk(case):
    """The same assertions where a workgroup streams two or three tiles of a chunk past its rows and carries their state from
    one to the next (what makes each case engage that carry: test_feature_metrics_host.test_large_cases_engage_the_tile_carry).
    The generated set's own scan has n_a = n_b > 1024: many row blocks, shared norms, the diagonal column in a later tile."""
    h = large_exact_case(case)
    m, k = len(h["fake"]), h["k"]
    cc = M.feature_scan_column_chunk(m)
    in_one_chunk, across_chunks = nearest_column_spread(h["rf"], k, cc)
    print(f"{LARGE_EXACT_CASES[case]}: chunk of {cc} columns ({cc // 64} tiles), {-(-m // cc)} chunks; rows with their k + 1 nearest "
          f"columns in >= 2 tiles of one chunk {int(in_one_chunk.sum())}, in >= 2 chunks {int(across_chunks.sum())} of {len(h['real'])}")
    assert cc > 64 and in_one_chunk.any() and across_chunks.any()
    _assert_scan_and_prdc_are_the_brute_force(LARGE_EXACT_CASES[case], h["real"], h["fake"], k, h["rr"], h["ff"], h["rf"])


def _assert_scan_and_prdc_are_the_brute_force(label, real, fake, k, rr, ff, rf):
    """real, fake: integer-valued sets; rr, ff, rf: their int64 squared distances.  Every output of the own-set scans, the
    cross scan with both radii, the reverse scan and prdc equals the brute force bit for bit."""
    n, m = len(real), len(fake)
    r_real, r_fake = np.sort(rr, 1)[:, k], np.sort(ff, 1)[:, k]
    ties = int((rf == r_real[:, None]).sum() + (rf == r_fake[None, :]).sum())
    print(f"{label}: {ties} squared distances equal a radius; largest squared distance {int(max(rr.max(), ff.max(), rf.max()))}")
    assert ties > 0 and max(rr.max(), ff.max()) < 2 ** 40
    R, F = _dev(real.astype(np.float64)), _dev(fake.astype(np.float64))

    own = M.feature_scan(R, R, k=k)
    assert own.kmin_sq.dtype == torch.float64 and tuple(own.kmin_sq.shape) == (n, k + 1)
    assert np.array_equal(_np(own.kmin_sq), np.sort(rr, 1)[:, :k + 1].astype(np.float64))
    assert np.array_equal(_np(own.min_sq), np.zeros(n)) and own.count_a is None and own.poly_sum is None
    assert np.array_equal(_np(M.knn_radii_sq(F, k=k)), r_fake.astype(np.float64))
    own = M.feature_scan(F, F, k=k)
    assert np.array_equal(_np(own.kmin_sq), np.sort(ff, 1)[:, :k + 1].astype(np.float64)) and np.array_equal(_np(own.min_sq), np.zeros(m))

    both = M.feature_scan(R, F, k=min(k, m - 1), radius_sq_a=_dev(r_real.astype(np.float64)), radius_sq_b=_dev(r_fake.astype(np.float64)))
    assert np.array_equal(_np(both.kmin_sq), np.sort(rf, 1)[:, :min(k, m - 1) + 1].astype(np.float64))
    assert both.count_a.dtype == torch.int32 and np.array_equal(_np(both.count_a), (rf < r_real[:, None]).sum(1))
    assert np.array_equal(_np(both.count_b), (rf < r_fake[None, :]).sum(1))
    assert np.array_equal(_np(both.min_sq), rf.min(1).astype(np.float64))
    back = M.feature_scan(F, R, radius_sq_b=_dev(r_real.astype(np.float64)))
    assert np.array_equal(_np(back.count_b), (rf < r_real[:, None]).sum(0)) and back.count_a is None and back.kmin_sq is None

    inside = rf < r_real[:, None]
    counts = {"precision_count": int(inside.any(0).sum()), "recall_count": int((rf < r_fake[None, :]).any(1).sum()),
              "density_count": int(inside.sum()), "coverage_count": int((rf.min(1) < r_real).sum())}
    got = M.prdc(R, F, k=k, return_terms=True)
    assert {name: got[name] for name in counts} == counts
    assert got["precision"] == counts["precision_count"] / m and got["recall"] == counts["recall_count"] / n
    assert got["density"] == counts["density_count"] / (k * m) and got["coverage"] == counts["coverage_count"] / n
    assert np.array_equal(_np(got["radius_sq_real"]), r_real.astype(np.float64))
    assert np.array_equal(_np(got["radius_sq_fake"]), r_fake.astype(np.float64))
    assert M.prdc(R, F, k=k) == {name: got[name] for name in ("precision", "recall", "density", "coverage")}
    assert M.prdc(R, F, k=k) == M.prdc_host(real, fake, k=k)


def test_single_element():
    a, b = _dev(np.array([[3.0]])), _dev(np.array([[-2.0]]))
    s = M.feature_scan(a, b)
    assert s.min_sq.tolist() == [25.0] and s.kmin_sq is None and s.count_a is None and s.count_b is None and s.poly_sum is None
    s = M.feature_scan(a, b, radius_sq_a=_dev(np.array([25.0])), radius_sq_b=_dev(np.array([26.0])), poly=True)
    assert s.count_a.tolist() == [0] and s.count_b.tolist() == [1]               # strict <
    assert s.poly_sum.tolist() == [(-6.0 + 1.0) ** 3]
    assert M.feature_scan(a, a, poly=True, exclude_diagonal=True).poly_sum.tolist() == [0.0]
    assert M.feature_scan(a, a, poly=True, exclude_diagonal=True, row_offset=1).poly_sum.tolist() == [1000.0]


def test_kernel_sums_are_exact_on_integer_features():
    rng = np.random.default_rng(64)
    x, y = rng.integers(-2, 3, (65, 64)).astype(np.float64), rng.integers(-2, 3, (33, 64)).astype(np.float64)
    X, Y = _dev(x), _dev(y)
    for (p, q, skip), (hp, hq) in zip(((X, X, True), (Y, Y, True), (X, Y, False), (Y, X, False)), ((x, x), (y, y), (x, y), (y, x))):
        got = M.feature_scan(p, q, poly=True, exclude_diagonal=skip).poly_sum
        want = M.feature_scan_host(hp, hq, poly=True, exclude_diagonal=skip).poly_sum
        g = hp @ hq.T
        t = (g / 64 + 1) ** 3
        brute = (t.sum(1) - (np.diag(t) if skip else 0.0))
        assert np.array_equal(_np(got), want) and np.array_equal(want, brute)
    got = M.kernel_distance(X, Y, return_terms=True)
    assert got == M.kernel_distance_host(x, y, return_terms=True) and got["krd"] == M.kernel_distance(X, Y)


def test_kernel_sums_are_exact_with_several_tiles_per_chunk():
    """1100 and 1300 rows: chunks of two tiles, the last one ragged, so a row's kernel sum is carried from tile to tile and the
    skipped diagonal column lies in a second tile for half of the rows.  d = 64, entries in -2 .. 2: t = m / 64 with m = g + 64
    an integer and t^3 = m^3 / 2^18, so a row sum is exact in any order while sum |m^3| stays below 2^53 -- asserted from the
    operands, in int64, before the device is touched."""
    rng = np.random.default_rng(65)
    xi, yi = rng.integers(-2, 3, (1100, 64)), rng.integers(-2, 3, (1300, 64))
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    cubes = {}
    for name, (p, q) in (("xx", (xi, xi)), ("yy", (yi, yi)), ("xy", (xi, yi)), ("yx", (yi, xi))):
        m3 = (p.astype(np.int64) @ q.astype(np.int64).T + 64) ** 3
        cubes[name] = m3
        print(f"{name}: largest |m| {int(np.cbrt(np.abs(m3).max()) + 0.5)}, largest row sum of |m^3| 2^{math.log2(np.abs(m3).sum(1).max()):.1f}")
        assert np.abs(m3).sum(1).max() < 2 ** 53
    assert M.feature_scan_column_chunk(1100) == 128 and M.feature_scan_column_chunk(1300) == 128
    X, Y = _dev(x), _dev(y)
    for name, p, q, hp, hq, skip in (("xx", X, X, x, x, True), ("yy", Y, Y, y, y, True), ("xy", X, Y, x, y, False), ("yx", Y, X, y, x, False),
                                     ("xx", X, X, x, x, False), ("yy", Y, Y, y, y, False)):
        got = _np(M.feature_scan(p, q, poly=True, exclude_diagonal=skip).poly_sum)
        want = M.feature_scan_host(hp, hq, poly=True, exclude_diagonal=skip).poly_sum
        m3 = cubes[name]
        brute = (m3.sum(1) - (np.diagonal(m3) if skip else 0)).astype(np.float64) / 2.0 ** 18         # exact: integers below 2^53
        print(f"{name} exclude_diagonal={skip}: {int((got != brute).sum())} of {len(brute)} row sums differ from the brute sum, "
              f"{int((want != brute).sum())} of the host statement's")
        assert np.array_equal(got, want) and np.array_equal(want, brute)
    got = M.kernel_distance(X, Y, return_terms=True)
    assert got == M.kernel_distance_host(x, y, return_terms=True) and got["krd"] == M.kernel_distance(X, Y)


# ---- properties -----------------------------------------------------------------------------------------------------------
def test_self_distance_is_exactly_zero():
    x = np.random.default_rng(7).normal(size=(70, 77))
    got = M.feature_scan(_dev(x), _dev(x), k=5)
    assert torch.equal(got.kmin_sq[:, 0], torch.zeros(70, dtype=torch.float64, device="cuda"))
    assert bool((got.kmin_sq[:, 1] > 0).all()) and torch.equal(got.min_sq, got.kmin_sq[:, 0])
    x[40] = x[3]
    got = M.feature_scan(_dev(x), _dev(x.copy()), k=5)                          # (two buffers: no shared norms)
    assert bool((got.kmin_sq[:, 0] == 0).all()) and got.kmin_sq[3, 1].item() == 0.0 and got.kmin_sq[40, 1].item() == 0.0
    assert int((got.kmin_sq[:, 1] == 0).sum()) == 2


def test_a_row_depends_on_itself_and_b_alone():
    rng = np.random.default_rng(8)
    a, b = _dev(rng.normal(size=(150, 77))), _dev(rng.normal(size=(150, 77)))                 # three column chunks, three row blocks
    ra, rb = _dev(rng.uniform(100.0, 200.0, 150)), _dev(rng.uniform(100.0, 200.0, 150))
    kw = dict(k=5, radius_sq_b=rb, poly=True, exclude_diagonal=True)
    whole = M.feature_scan(a, b, radius_sq_a=ra, **kw)
    assert 0 < int(whole.count_a.sum()) < 150 * 150 and 0 < int(whole.count_b.sum()) < 150 * 150
    for lo, hi in ((3, 9), (60, 131), (149, 150)):
        part = M.feature_scan(a[lo:hi], b, radius_sq_a=ra[lo:hi], row_offset=lo, **kw)
        _same_scan(part, M.FeatureScan(*[getattr(whole, name)[lo:hi] for name in OUTPUTS]))
    _same_scan(M.feature_scan(a, b, radius_sq_a=ra, **kw), whole)               # two calls agree bit for bit
    # the diagonal is a matter of row_offset alone: without it, the slice's rows skip other columns
    kept = M.feature_scan(a, b, poly=True).poly_sum
    assert not torch.equal(kept, whole.poly_sum)
    t = (a[5] @ b[5]).item() / 77 + 1.0
    assert abs((kept[5] - whole.poly_sum[5]).item() - t * t * t) <= 1e-9 * abs(kept[5].item())


def test_a_row_depends_on_itself_and_b_alone_with_several_tiles_per_chunk():
    """The same promise at n_b = 1100: nine chunks of two tiles.  The slices start inside a row block, and the skipped diagonal
    column of rows 64 .. 127 and of row 1099 lies in the second tile of its chunk."""
    rng = np.random.default_rng(9)
    n = 1100
    a, b = _dev(rng.normal(size=(n, 77))), _dev(rng.normal(size=(n, 77)))
    ra, rb = _dev(rng.uniform(100.0, 200.0, n)), _dev(rng.uniform(100.0, 200.0, n))
    kw = dict(k=16, radius_sq_b=rb, poly=True, exclude_diagonal=True)
    whole = M.feature_scan(a, b, radius_sq_a=ra, **kw)
    print(f"count_a sums to {int(whole.count_a.sum())}, count_b to {int(whole.count_b.sum())} of {n * n}")
    assert 0 < int(whole.count_a.sum()) < n * n and 0 < int(whole.count_b.sum()) < n * n
    for lo, hi in ((3, 9), (60, 131), (1099, 1100)):
        part = M.feature_scan(a[lo:hi], b, radius_sq_a=ra[lo:hi], row_offset=lo, **kw)
        _same_scan(part, M.FeatureScan(*[getattr(whole, name)[lo:hi] for name in OUTPUTS]))
    _same_scan(M.feature_scan(a, b, radius_sq_a=ra, **kw), whole)               # two calls agree bit for bit
    kept = M.feature_scan(a, b, poly=True).poly_sum
    differ = (kept != whole.poly_sum).cpu().numpy()
    print(f"{int(differ.sum())} of {n} row sums change when the diagonal column is kept")
    assert differ[[5, 70, 1099]].all()                   # (70, 1099: the second tile of chunks 0 and 8)


# ---- real-valued, against the numpy statement -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host(i):
    """Case i's inputs, numpy statements and bounds, computed once."""
    real, fake, k = real_case(i)
    d = real.shape[1]
    s_r, s_f = (real * real).sum(1), (fake * fake).sum(1)
    scale = 4 * (d + 2) * EPS
    out = {"real": real, "fake": fake, "k": k, "d": d,
           "rr": M.feature_scan_host(real, real, k=k), "ff": M.feature_scan_host(fake, fake, k=k),
           "bound_rr": scale * (s_r + s_r.max()), "bound_ff": scale * (s_f + s_f.max()),
           "bound_rf": scale * (s_r[:, None] + s_f[None, :])}
    r_real, r_fake = out["rr"].kmin_sq[:, k], out["ff"].kmin_sq[:, k]
    out["rf"] = M.feature_scan_host(real, fake, k=k, radius_sq_a=r_real, radius_sq_b=r_fake)
    out["fr"] = M.feature_scan_host(fake, real, radius_sq_b=r_real)
    g = real @ fake.T
    d2 = np.maximum(0.0, (s_r[:, None] + s_f[None, :]) - 2.0 * g)
    near = (np.abs(d2 - r_real[:, None]) <= out["bound_rf"] + out["bound_rr"][:, None]).sum()
    near += (np.abs(d2 - r_fake[None, :]) <= out["bound_rf"] + out["bound_ff"][None, :]).sum()
    out["near_ties"] = int(near)
    return out


def _poly_bound(a, b, skip_diagonal):
    """Per row: the sum over j of 3 t^2 |dg| / d + 4 2^-52 |t^3| with |dg| <= d 2^-52 sum |a| |b|."""
    d = a.shape[1]
    t = (a @ b.T) / d + 1.0
    dg = d * EPS * (np.abs(a) @ np.abs(b).T)
    term = 3.0 * t * t * dg / d + 4.0 * EPS * np.abs(t * t * t)
    if skip_diagonal:
        np.fill_diagonal(term, 0.0)
    return term.sum(1)


@pytest.mark.parametrize("i", range(len(REAL_SHAPES)), ids=[str(c) for c in REAL_SHAPES])
def test_real_valued_scan_against_the_numpy_statement(i):
    h = _host(i)
    k = h["k"]
    assert h["near_ties"] == 0                           # numpy alone: no comparison of this case can go either way
    R, F = _dev(h["real"]), _dev(h["fake"])
    worst = 0.0
    for a, b, name in ((R, R, "rr"), (F, F, "ff")):
        got = M.feature_scan(a, b, k=k)
        ratio = np.abs(_np(got.kmin_sq) - h[name].kmin_sq) / h["bound_" + name][:, None]
        worst = max(worst, float(ratio.max()))
        assert torch.equal(got.kmin_sq[:, 0], torch.zeros_like(got.min_sq))
    r_real, r_fake = M.knn_radii_sq(R, k=k), M.knn_radii_sq(F, k=k)
    got = M.feature_scan(R, F, k=k, radius_sq_a=r_real, radius_sq_b=r_fake)
    row_bound = h["bound_rf"].max(1)
    worst = max(worst, float((np.abs(_np(got.kmin_sq) - h["rf"].kmin_sq) / row_bound[:, None]).max()),
                float((np.abs(_np(got.min_sq) - h["rf"].min_sq) / row_bound).max()))
    print(f"case {i} {REAL_SHAPES[i]}: worst squared-distance difference / bound {worst:.3g}")
    assert worst <= 1.0
    assert np.array_equal(_np(got.count_a), h["rf"].count_a) and np.array_equal(_np(got.count_b), h["rf"].count_b)
    back = M.feature_scan(F, R, radius_sq_b=r_real)
    assert np.array_equal(_np(back.count_b), h["fr"].count_b)
    assert M.prdc(R, F, k=k) == M.prdc_host(h["real"], h["fake"], k=k)
    terms, want = M.prdc(R, F, k=k, return_terms=True), M.prdc_host(h["real"], h["fake"], k=k, return_terms=True)
    assert all(terms[c] == want[c] for c in ("precision_count", "recall_count", "density_count", "coverage_count"))


@pytest.mark.parametrize("i", range(len(REAL_SHAPES)), ids=[str(c) for c in REAL_SHAPES])
def test_real_valued_kernel_sums_against_the_numpy_statement(i):
    h = _host(i)
    worst = 0.0
    for a, b, skip in ((h["real"], h["real"], True), (h["fake"], h["fake"], True), (h["real"], h["fake"], False)):
        got = _np(M.feature_scan(_dev(a), _dev(b), poly=True, exclude_diagonal=skip).poly_sum)
        want = M.feature_scan_host(a, b, poly=True, exclude_diagonal=skip).poly_sum
        worst = max(worst, float((np.abs(got - want) / _poly_bound(a, b, skip)).max()))
    print(f"case {i} {REAL_SHAPES[i]}: worst kernel row sum difference / bound {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("i", (0, 1, 3), ids=[str(REAL_SHAPES[c]) for c in (0, 1, 3)])
def test_scan_is_the_fold_of_gram_f64_bit_for_bit(i):
    """feature_scan's documented promise on real-valued data, where the summation order shows: its g is gram_f64's value and
    its s the diagonal of gram_f64(x, x), so the numpy fold over those (nothing else in it rounds differently) gives every
    output bit for bit.  The cases hold a ragged row tile and a ragged column tile, d no multiple of 32 nor of 4, one column
    chunk (n_b = 63, 64) and three with the merge kernel (n_b = 150)."""
    _assert_scan_is_the_fold_of_gram_f64(*real_case(i))


def test_scan_is_the_fold_of_gram_f64_with_several_tiles_per_chunk():
    """The same at n_b = 1100 and k = FEATURE_K_CAP: nine chunks of two tiles (the last one ragged), the list of smallest
    values completely full.  On real values the order of the additions shows, so poly_sum pins the carry of a row's sum from
    one tile of a chunk to the next: ascending j within the chunk, then ascending chunks."""
    real, fake, k = real_inputs(LARGE_REAL_SHAPE, 4)
    assert M.feature_scan_column_chunk(len(fake)) == 128 and k == M.FEATURE_K_CAP
    _assert_scan_is_the_fold_of_gram_f64(real, fake, k)
    _assert_scan_is_the_fold_of_gram_f64(fake, real, k)  # the 1100 rows against themselves, the diagonal skipped in later tiles


def _assert_scan_is_the_fold_of_gram_f64(real, fake, k):
    d = real.shape[1]
    A, B = _dev(real), _dev(fake)
    g_ab, g_aa, g_bb = (_np(M.gram_f64(p, q)) for p, q in ((A, B), (A, A), (B, B)))
    s_a, s_b = g_aa.diagonal().copy(), g_bb.diagonal().copy()
    own_a = M._scan_fold_host(g_aa, s_a, s_a, d, k, None, None, True, True, 0)
    own_b = M._scan_fold_host(g_bb, s_b, s_b, d, k, None, None, False, False, 0)
    ra, rb = own_a.kmin_sq[:, k].copy(), own_b.kmin_sq[:, k].copy()
    want = M._scan_fold_host(g_ab, s_a, s_b, d, k, ra, rb, True, False, 0)
    got = M.feature_scan(A, B, k=k, radius_sq_a=_dev(ra), radius_sq_b=_dev(rb), poly=True)
    own = M.feature_scan(A, A, k=k, poly=True, exclude_diagonal=True)
    shape = f"({len(real)}, {len(fake)}, {d}, {k})"
    print(f"{shape}: values that differ from the fold: " + ", ".join(f"{name} {int((_np(getattr(got, name)) != getattr(want, name)).sum())}" for name in OUTPUTS)
          + "; own set: " + ", ".join(f"{name} {int((_np(getattr(own, name)) != getattr(own_a, name)).sum())}" for name in ("kmin_sq", "min_sq", "poly_sum")))
    for name in OUTPUTS:
        assert np.array_equal(_np(getattr(got, name)), getattr(want, name)), name
    assert own.count_a is None and own.count_b is None
    for name in ("kmin_sq", "min_sq", "poly_sum"):
        assert np.array_equal(_np(getattr(own, name)), getattr(own_a, name)), name


# ---- kernel distance ------------------------------------------------------------------------------------------------------
def test_kernel_distance_against_the_numpy_statement_and_over_subsets():
    h = _host(0)
    x, y = h["fake"], h["real"]
    n1, n2 = len(x), len(y)
    X, Y = _dev(x), _dev(y)
    got, want = M.kernel_distance(X, Y), M.kernel_distance_host(x, y)
    bound = (_poly_bound(x, x, True).sum() / (n1 * (n1 - 1)) + _poly_bound(y, y, True).sum() / (n2 * (n2 - 1))
             + 2.0 * _poly_bound(x, y, False).sum() / (n1 * n2))
    print(f"krd {got!r}, numpy statement {want!r}, difference / bound {abs(got - want) / bound:.3g}")
    assert abs(got - want) <= bound
    assert M.kernel_distance(X, Y) == got
    sub = M.kernel_distance(X, Y, subset_size=40, subsets=5, seed=2, return_terms=True)
    rows_x, rows_y = M.kernel_subsets(n1, 40, 5, 2, 0), M.kernel_subsets(n2, 40, 5, 2, 1)
    estimates = [M.kernel_distance(_dev(x[rows_x[s]]), _dev(y[rows_y[s]])) for s in range(5)]
    assert sub["estimates"] == estimates and (sub["subsets"], sub["subset_size"]) == (5, 40)
    mean = math.fsum(estimates) / 5
    assert sub["krd"] == mean and sub["krd_std"] == math.sqrt(math.fsum((e - mean) ** 2 for e in estimates) / 5)
    assert sub["krd"] == pytest.approx(np.mean(estimates), rel=1e-13) and sub["krd_std"] == pytest.approx(np.std(estimates), rel=1e-12)
    assert M.kernel_distance(X, Y, subset_size=40, subsets=5, seed=2) == {"krd": sub["krd"], "krd_std": sub["krd_std"]}


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path():
    rng = np.random.default_rng(22)
    x32, y32 = _dev(rng.normal(size=(20, 24)).astype(np.float32)), _dev(rng.normal(size=(17, 24)).astype(np.float32))
    want = M.prdc(x32.double(), y32.double(), k=3)
    assert M.prdc(x32, y32, k=3) == want and M.prdc(x32, y32.double(), k=3) == want          # any float dtype
    bad = y32.clone()
    bad[5, 7] = float("inf")
    for call in (lambda: M.feature_scan(x32, bad), lambda: M.feature_scan(bad, x32, k=2), lambda: M.knn_radii_sq(bad, k=2),
                 lambda: M.prdc(x32, bad, k=3), lambda: M.prdc(bad, x32, k=3), lambda: M.kernel_distance(x32, bad),
                 lambda: M.feature_scan(x32, y32, radius_sq_b=torch.full((17,), float("nan"), device="cuda"))):
        with pytest.raises(ValueError, match="NaN or inf"):
            call()
    assert M.prdc(x32, y32, k=3) == want                                          # and the next call is what it was
    for call in (lambda: M.feature_scan(x32.cpu(), y32.cpu()), lambda: M.prdc(x32.cpu(), y32, k=3),
                 lambda: M.kernel_distance(x32, y32.cpu()), lambda: M.knn_radii_sq(x32.cpu(), k=2)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    with pytest.raises(ValueError):
        M.prdc(x32, y32, k=M.FEATURE_K_CAP + 1)


# ---- the driver -------------------------------------------------------------------------------------------------------------
def test_evaluate_features_one_process_and_two_ranks(tmp_path):
    from rangeldm_amd import evaluate as E
    rng = np.random.default_rng(41)
    total, count = 512, 64
    folders = []
    for name, files, shift in (("gen", 12, 0.3), ("ref", 9, 0.0)):
        d = tmp_path / name
        d.mkdir()
        for i in range(files):
            np.save(str(d / f"{i:03d}.npy"), rng.normal(shift, 1.0, (8, 8, 8)).astype(np.float32))
        folders.append(str(d))
    out = tmp_path / "features.json"
    size = ["--total", str(total), "--count", str(count)]
    args = ["features", *folders, "--k", "3", *size]
    one = _run_evaluate(1, args + ["--json", str(out)], timeout=300)
    res = json.loads(one)
    assert set(res) == {"task", "krd", "precision", "recall", "density", "coverage", "k", "n_gen", "n_ref", "dims"}
    assert (res["task"], res["k"], res["n_gen"], res["n_ref"], res["dims"]) == ("features", 3, 12, 9, count)
    assert out.read_text() == one + "\n"
    idx = M.frd_indices(total, count)
    gen, ref = (M.load_activations(f, idx, limit=None, total=total) for f in folders)
    assert tuple(gen.shape) == (12, count) and tuple(ref.shape) == (9, count)
    assert res["krd"] == M.kernel_distance(gen, ref)
    assert {name: res[name] for name in ("precision", "recall", "density", "coverage")} == M.prdc(ref, gen, k=3)
    # --limit and the subset options, in this process: the object the command would print
    a = E.build_parser().parse_args(args + ["--limit", "8", "--subset-size", "6", "--subsets", "4", "--seed", "5"])
    sub = E.cmd_features(a, 0, 1, torch.device("cuda", torch.cuda.current_device()))
    assert set(sub) == set(res) | {"krd_std", "subsets", "subset_size"} and (sub["n_gen"], sub["n_ref"]) == (8, 8)
    want = M.kernel_distance(gen[:8], ref[:8], subset_size=6, subsets=4, seed=5)
    assert (sub["krd"], sub["krd_std"], sub["subsets"], sub["subset_size"]) == (want["krd"], want["krd_std"], 4, 6)
    assert {name: sub[name] for name in ("precision", "recall", "density", "coverage")} == M.prdc(ref[:8], gen[:8], k=3)
    for wrong in (["--k", "0"], ["--k", "17"], ["--limit", "3"], ["--subset-size", "1"], ["--projection", "device"]):
        with pytest.raises(ValueError):
            E.check_features_args(E.build_parser().parse_args(args + wrong))
    # `frd` on the same folders prints what it printed before
    frd = json.loads(_run_evaluate(1, ["frd", *folders, *size], timeout=300))
    want = M.frechet_distance(gen, ref, return_terms=True)
    assert set(frd) == {"task", "frd", "mean_sq", "tr1", "tr2", "tr_sqrt", "sweeps", "n1", "n2", "dims"}
    assert {name: frd[name] for name in want} == want and (frd["n1"], frd["n2"], frd["dims"]) == (12, 9, count)
    # (only now, after the first launches succeeded) two ranks: rank 0 alone computes, the output is byte-identical
    assert _run_evaluate(2, args, timeout=300) == one
