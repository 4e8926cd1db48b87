"""The numpy statements of the feature-space metrics (rangeldm_amd.metrics.feature_scan_host / prdc_host /
kernel_distance_host / kernel_subsets) against independent forms, on the CPU.

prdc_host is held against the form of the `prdc` package (Naeem et al. 2020), restated from the papers:
scipy.spatial.distance.cdist (unsquared Euclidean distances), np.argpartition for the (k + 1)-th smallest value of a row,
and `<`.  The comparison is on the integer counts, so it is exact.  kernel_distance_host is held against
sklearn.metrics.pairwise.polynomial_kernel(degree=3, coef0=1) (gamma defaults to 1 / d) with KID's unbiased estimator.

real_case(i) are the real-valued inputs tests/test_feature_metrics_gpu.py holds the device to as well.

Several tiles per column chunk.  feature_scan_column_chunk(n_b) is 64, one tile, for every n_b <= 1024; only above that does
a workgroup of the device's scan carry a row's state (its k + 1 smallest values, the counts, the minimum, the kernel sum) from
one tile of 64 columns to the next.  LARGE_EXACT_CASES are integer-valued inputs with 1025 .. 2049 generated rows (two and
three tiles per chunk, a last chunk of one column, of a ragged second tile, of a third tile that holds one column, and a full
one) and k up to FEATURE_K_CAP.  test_large_cases_engage_the_tile_carry asserts, on numpy alone, what makes them worth
running on the device: radius ties, rows whose k + 1 nearest columns lie in two or more tiles of ONE chunk (the values a
workgroup must carry) and in two chunks (the merge), and that feature_scan_host is the int64 brute force on them.
"""
import functools
import math

import numpy as np
import pytest

from rangeldm_amd import metrics as M

REAL_SHAPES = [(65, 63, 33, 5), (130, 64, 259, 5), (17, 33, 5, 1), (200, 150, 64, 3)]        # (N, M, d, k)
LARGE_REAL_SHAPE = (70, 1100, 37, 16)                    # two tiles per chunk, the last chunk ragged; k = FEATURE_K_CAP
LARGE_EXACT_CASES = [(70, 1025, 8, 5, 2), (130, 1100, 33, 16, 3), (65, 2049, 16, 16, 2), (64, 1664, 12, 1, 2)]   # (N, M, d, k, L)
TILE = 64                                                # columns per tile of the device's scan


def real_inputs(shape, seed):
    """(real, generated, k) for (N, M, d, k): rng = default_rng(seed), real = rng.normal, generated = rng.normal * 0.8 + 0.3."""
    n, m, d, k = shape
    rng = np.random.default_rng(seed)
    real = rng.normal(size=(n, d))
    fake = rng.normal(size=(m, d)) * 0.8 + 0.3
    return real, fake, k


def real_case(i):
    """(real, generated, k) of case i: real_inputs(REAL_SHAPES[i], seed i)."""
    return real_inputs(REAL_SHAPES[i], i)


def exact_inputs(shape, seed):
    """(real, generated, k) for (N, M, d, k, L): integer entries in -L .. L, one real row duplicating its neighbour and three
    generated rows equal to real rows."""
    n, m, d, k, lim = shape
    rng = np.random.default_rng(seed)
    real = rng.integers(-lim, lim + 1, (n, d))
    fake = rng.integers(-lim, lim + 1, (m, d))
    real[n // 3 + 1] = real[n // 3]                      # one real row duplicates its neighbour
    fake[[0, m // 2, m - 1]] = real[[0, n // 2, n - 1]]  # three generated rows equal real rows
    return real, fake, k


def brute_sq(a, b):
    """All squared distances of integer rows as int64 (n_a, n_b), by the exact integer identity |a|^2 + |b|^2 - 2 a.b: no
    (n_a, n_b, d) temporary."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)


@functools.lru_cache(maxsize=None)
def large_exact_case(case):
    """Large case `case`, computed once and left unchanged: real, fake, k, the three int64 distance matrices, both radius
    vectors and the number of squared distances that equal a radius."""
    real, fake, k = exact_inputs(LARGE_EXACT_CASES[case], 200 + case)
    rr, ff, rf = brute_sq(real, real), brute_sq(fake, fake), brute_sq(real, fake)
    r_real, r_fake = np.sort(rr, 1)[:, k], np.sort(ff, 1)[:, k]
    ties = int((rf == r_real[:, None]).sum() + (rf == r_fake[None, :]).sum())
    out = {"real": real, "fake": fake, "k": k, "rr": rr, "ff": ff, "rf": rf, "r_real": r_real, "r_fake": r_fake, "ties": ties}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def nearest_column_spread(d2, k, chunk_cols):
    """For every row of d2, where its k + 1 nearest columns (stable order) lie: (rows with two or more tiles of one chunk
    among them, rows with two or more chunks among them), as boolean vectors."""
    near = np.argsort(d2, axis=1, kind="stable")[:, :k + 1]
    tiles, chunks = near // TILE, near // chunk_cols
    in_one_chunk = np.zeros(d2.shape[0], bool)
    for c in range(-(-d2.shape[1] // chunk_cols)):
        held = np.where(chunks == c, tiles, -1)          # the tiles of chunk c among the row's nearest, -1 elsewhere
        top = held.max(1, keepdims=True)
        in_one_chunk |= ((held >= 0) & (held != top)).any(1)
    across_chunks = (chunks != chunks[:, :1]).any(1)
    return in_one_chunk, across_chunks


def prdc_counts_independent(real, fake, k):
    """The `prdc` package's compute_prdc, kept as integer counts: (precision, recall, density, coverage) numerators."""
    from scipy.spatial.distance import cdist

    def kth(dist):                                       # get_kth_value(dist, k + 1): the largest of the k + 1 smallest
        idx = np.argpartition(dist, k, axis=-1)[..., :k + 1]
        return np.take_along_axis(dist, idx, axis=-1).max(axis=-1)

    r_real, r_fake = kth(cdist(real, real)), kth(cdist(fake, fake))
    dist = cdist(real, fake)
    inside_real = dist < r_real[:, None]
    return (int(inside_real.any(axis=0).sum()), int((dist < r_fake[None, :]).any(axis=1).sum()), int(inside_real.sum()),
            int((dist.min(axis=1) < r_real).sum()))


def krd_independent(x, y):
    from sklearn.metrics.pairwise import polynomial_kernel
    kxx, kyy, kxy = (polynomial_kernel(p, q, degree=3, coef0=1) for p, q in ((x, x), (y, y), (x, y)))
    n1, n2 = len(x), len(y)
    return ((kxx.sum() - np.trace(kxx)) / (n1 * (n1 - 1)) + (kyy.sum() - np.trace(kyy)) / (n2 * (n2 - 1))
            - 2.0 * kxy.sum() / (n1 * n2))


@pytest.mark.parametrize("i", range(len(REAL_SHAPES)))
def test_prdc_host_equals_the_cdist_form(i):
    real, fake, k = real_case(i)
    got = M.prdc_host(real, fake, k=k, return_terms=True)
    want = prdc_counts_independent(real, fake, k)
    n, m = len(real), len(fake)
    assert (got["precision_count"], got["recall_count"], got["density_count"], got["coverage_count"]) == want
    assert got["precision"] == want[0] / m and got["recall"] == want[1] / n
    assert got["density"] == want[2] / (k * m) and got["coverage"] == want[3] / n
    assert set(M.prdc_host(real, fake, k=k)) == {"precision", "recall", "density", "coverage"}
    radii = M.feature_scan_host(real, real, k=k).kmin_sq[:, k]
    assert np.array_equal(got["radius_sq_real"], radii) and got["radius_sq_fake"].shape == (m,)


@pytest.mark.parametrize("i", range(len(REAL_SHAPES)))
def test_kernel_distance_host_equals_the_sklearn_form(i):
    real, fake, _ = real_case(i)
    got, want = M.kernel_distance_host(fake, real), krd_independent(fake, real)
    print(f"case {i}: krd {got!r}, sklearn form {want!r}, relative difference {abs(got - want) / abs(want):.3g}")
    assert abs(got - want) <= 1e-12 * abs(want)
    terms = M.kernel_distance_host(fake, real, return_terms=True)
    assert terms["krd"] == got and set(terms) == {"krd", "sum_xx", "sum_yy", "sum_xy"}


def test_feature_scan_host_outputs():
    rng = np.random.default_rng(11)
    a, b = rng.integers(-3, 4, (9, 6)).astype(np.float64), rng.integers(-3, 4, (150, 6)).astype(np.float64)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    ra, rb = np.full(9, 20.0), rng.integers(5, 30, 150).astype(np.float64)
    s = M.feature_scan_host(a, b, k=4, radius_sq_a=ra, radius_sq_b=rb, poly=True)
    assert np.array_equal(s.kmin_sq, np.sort(d2, 1)[:, :5]) and np.array_equal(s.min_sq, d2.min(1))
    assert np.array_equal(s.count_a, (d2 < 20).sum(1)) and np.array_equal(s.count_b, (d2 < rb[None]).sum(1))
    assert s.count_a.dtype == np.int32
    kappa = (a @ b.T / 6 + 1) ** 3
    assert np.allclose(s.poly_sum, kappa.sum(1), rtol=1e-13, atol=0)
    skipped = M.feature_scan_host(a[2:5], b, poly=True, exclude_diagonal=True, row_offset=2)
    assert np.allclose(skipped.poly_sum, [kappa[i].sum() - kappa[i, i] for i in (2, 3, 4)], rtol=1e-12, atol=0)
    assert skipped.kmin_sq is None and skipped.count_a is None and skipped.count_b is None
    # the column chunk: a function of n_b alone, at most 16 chunks of a multiple of 64 rows
    assert [M.feature_scan_column_chunk(n) for n in (1, 64, 65, 1024, 1025, 10000, 50000)] == [64, 64, 64, 64, 128, 640, 3136]


@pytest.mark.parametrize("case", range(len(LARGE_EXACT_CASES)), ids=[str(c) for c in LARGE_EXACT_CASES])
def test_large_cases_engage_the_tile_carry(case):
    """What makes a large case worth running on the device, asserted on numpy alone, and feature_scan_host against the int64
    brute force on it (kmin_sq, count_a, count_b, min_sq: the outputs that are exact here; d is no power of two, so t is not)."""
    n, m, d, k, lim = LARGE_EXACT_CASES[case]
    h = large_exact_case(case)
    real, fake, rr, ff, rf, r_real, r_fake = (h[name] for name in ("real", "fake", "rr", "ff", "rf", "r_real", "r_fake"))
    cc = M.feature_scan_column_chunk(m)
    chunks = -(-m // cc)
    in_one_chunk, across_chunks = nearest_column_spread(rf, k, cc)
    own_one, own_across = nearest_column_spread(ff, k, cc)
    largest = int(max(rr.max(), ff.max(), rf.max()))
    print(f"{LARGE_EXACT_CASES[case]}: chunk of {cc} columns, {chunks} chunks, the last of {m - (chunks - 1) * cc}; {h['ties']} squared "
          f"distances equal a radius; largest squared distance {largest}; rows with their k + 1 nearest generated columns in >= 2 "
          f"tiles of one chunk {int(in_one_chunk.sum())} of {n}, in >= 2 chunks {int(across_chunks.sum())} of {n}; generated rows "
          f"against their own set: {int(own_one.sum())} and {int(own_across.sum())} of {m}")
    assert cc > TILE and chunks > 1 and cc % TILE == 0 and chunks <= 16
    assert h["ties"] > 0 and largest < 2 ** 40
    assert in_one_chunk.any() and across_chunks.any()
    if case < 3:
        assert 4 * int(in_one_chunk.sum()) >= n
    assert (np.diagonal(rr) == 0).all() and (np.diagonal(ff) == 0).all() and rf.min() == 0
    assert np.array_equal(rf[:4], ((real[:4, None, :] - fake[None, :, :]) ** 2).sum(-1))       # the identity, on a row block

    f64 = lambda a: a.astype(np.float64)
    own = M.feature_scan_host(f64(real), f64(real), k=k)
    assert np.array_equal(own.kmin_sq, f64(np.sort(rr, 1)[:, :k + 1])) and np.array_equal(own.min_sq, np.zeros(n))
    own = M.feature_scan_host(f64(fake), f64(fake), k=k)
    assert np.array_equal(own.kmin_sq, f64(np.sort(ff, 1)[:, :k + 1])) and np.array_equal(own.min_sq, np.zeros(m))
    both = M.feature_scan_host(f64(real), f64(fake), k=k, radius_sq_a=f64(r_real), radius_sq_b=f64(r_fake))
    assert np.array_equal(both.kmin_sq, f64(np.sort(rf, 1)[:, :k + 1])) and np.array_equal(both.min_sq, f64(rf.min(1)))
    assert np.array_equal(both.count_a, (rf < r_real[:, None]).sum(1)) and np.array_equal(both.count_b, (rf < r_fake[None, :]).sum(1))
    back = M.feature_scan_host(f64(fake), f64(real), k=k, radius_sq_a=f64(r_fake), radius_sq_b=f64(r_real))
    assert np.array_equal(back.kmin_sq, f64(np.sort(rf.T, 1)[:, :k + 1])) and np.array_equal(back.min_sq, f64(rf.min(0)))
    assert np.array_equal(back.count_a, (rf < r_fake[None, :]).sum(0)) and np.array_equal(back.count_b, (rf < r_real[:, None]).sum(0))


def test_kernel_subsets_is_reproducible_and_distinct():
    import random
    a = M.kernel_subsets(50, 20, 6, 3, 0)
    assert a == M.kernel_subsets(50, 20, 6, 3, 0)
    assert a[2] == random.Random(3 + 4).sample(range(50), 20)
    b = M.kernel_subsets(50, 20, 6, 3, 1)
    assert b[2] == random.Random(3 + 5).sample(range(50), 20)
    draws = [tuple(r) for r in a + b]
    assert len(set(draws)) == 12                         # every s, and x against y, draws its own rows
    assert all(len(set(r)) == 20 and 0 <= min(r) and max(r) < 50 for r in draws)
    rng = np.random.default_rng(5)
    x, y = rng.normal(size=(50, 7)), rng.normal(size=(40, 7)) + 0.5
    got = M.kernel_distance_host(x, y, subset_size=20, subsets=6, seed=3, return_terms=True)
    rows_y = M.kernel_subsets(40, 20, 6, 3, 1)
    want = [M.kernel_distance_host(x[a[s]], y[rows_y[s]]) for s in range(6)]
    assert got["estimates"] == want and (got["subsets"], got["subset_size"]) == (6, 20)
    assert got["krd"] == math.fsum(want) / 6
    assert got["krd_std"] == pytest.approx(np.std(want), rel=1e-12)
    assert set(M.kernel_distance_host(x, y, subset_size=20, subsets=6, seed=3)) == {"krd", "krd_std"}


def test_known_answers():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(120, 16))
    same = M.prdc_host(x, x.copy(), k=5)
    assert same == {"precision": 1.0, "recall": 1.0, "density": 1.0, "coverage": 1.0}
    far = M.prdc_host(x, x + 100.0, k=5)
    assert far == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    # a real set of two clusters 20 apart, a generated set on one of them: faithful, but half of the data is never produced
    real = rng.normal(size=(200, 16))
    real[100:, 0] += 20.0
    fake = rng.normal(size=(200, 16))
    one = M.prdc_host(real, fake, k=5)
    print(one)
    assert one["precision"] > 0.9 and one["recall"] < 0.5 and abs(one["coverage"] - 0.5) <= 0.05
    # the unbiased estimate is not clamped: a set against itself leaves the diagonal out of the self terms only, so it is < 0
    assert M.kernel_distance_host(x, x.copy()) < 0.0
    again = rng.normal(size=(120, 16))
    assert abs(M.kernel_distance_host(x, again)) < M.kernel_distance_host(x, again + 1.0)


def test_value_errors():
    x, y = np.zeros((8, 4)), np.zeros((9, 4))
    for scan_args in (dict(a=np.zeros(8), b=y), dict(a=x, b=np.zeros((9, 5))), dict(a=x, b=y, k=0), dict(a=x, b=y, k=17),
                      dict(a=x, b=y, k=9), dict(a=x, b=y, radius_sq_a=np.zeros(9)), dict(a=x, b=y, radius_sq_b=np.zeros(8)),
                      dict(a=x, b=y, row_offset=-1), dict(a=np.zeros((0, 4)), b=y)):
        with pytest.raises(ValueError):
            M.feature_scan_host(**scan_args)
    assert M.feature_scan_host(x, y, k=8).kmin_sq.shape == (8, 9)                # n_b = k + 1 is enough
    assert M.FEATURE_K_CAP >= 16
    for k in (0, M.FEATURE_K_CAP + 1, 8):                                        # 8: the smaller set has 8 < k + 1 rows
        with pytest.raises(ValueError):
            M.prdc_host(x, y, k=k)
    with pytest.raises(ValueError):
        M.prdc_host(x, np.zeros((9, 5)))
    for args in ((np.zeros((1, 4)), y), (x, np.zeros((1, 4))), (x, np.zeros((9, 3)))):
        with pytest.raises(ValueError):
            M.kernel_distance_host(*args)
    for kw in (dict(subset_size=9), dict(subset_size=1), dict(subset_size=4, subsets=0)):
        with pytest.raises(ValueError):
            M.kernel_distance_host(x, y, **kw)
    for args in ((8, 9, 3, 0, 0), (8, 4, 3, 0, 2), (8, 1, 3, 0, 0), (8, 4, 0, 0, 0)):
        with pytest.raises(ValueError):
            M.kernel_subsets(*args)


def test_device_functions_refuse_before_the_device_is_looked_at():
    """The same ValueErrors from the device entry points, raised on host tensors: the checks run before anything asks for a
    GPU (a host tensor that passes them is a RuntimeError, tests/test_feature_metrics_gpu.py)."""
    import torch
    x, y = torch.zeros((8, 4)), torch.zeros((9, 4))
    for scan_args in (dict(a=x, b=torch.zeros((9, 5))), dict(a=x, b=y, k=0), dict(a=x, b=y, k=17), dict(a=x, b=y, k=9),
                      dict(a=x, b=y, radius_sq_a=torch.zeros(9)), dict(a=x.long(), b=y), dict(a=x, b=y, row_offset=-1)):
        with pytest.raises(ValueError):
            M.feature_scan(**scan_args)
    with pytest.raises(ValueError):
        M.knn_radii_sq(x, k=8)
    for k in (0, 17, 8):
        with pytest.raises(ValueError):
            M.prdc(x, y, k=k)
    with pytest.raises(ValueError):
        M.kernel_distance(torch.zeros((1, 4)), y)
    with pytest.raises(ValueError):
        M.kernel_distance(x, y, subset_size=9)
