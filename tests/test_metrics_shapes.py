"""metrics.hip away from bins = 100: the BEV histogram, the spectral norm, JSD and MMD at the smallest and the largest grids
the kernels take, at set sizes nx != ny, and with points planted on, just below and just above every bin edge.

Tolerances are the project's own (tests/test_metrics.py): histogram counts bit-exact, spectral norm squared 1e-4 relative,
JSD 1e-12, MMD terms 1e-8 and their combination 2e-4 relative.  The references are numpy: np.histogramdd through
oracle.metrics, np.linalg.svd, and an fp64 statement of the Jensen-Shannon distance with rel_entr written out.
"""
import numpy as np
import pytest
import torch

from oracle import metrics as om

F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- histogram ------------------------------------------------------------------------------------------------------
HIST_CASES = [(160, 2), (7.0, 6), (160, 10), (50.0, 104)]


def hist_clouds(field, bins, seed=0):
    """Four clouds (n_i, 4) fp32, the first one empty.  Cloud 1: every pair (x, y) of edge values -- each bin edge as
    fp32, one ulp below and one ulp above it, -half and +half included -- and the same values against points outside the
    field.  Cloud 2: 777 random points, a third of them outside.  Cloud 3: more than 64 * 256 points (the kernel's grid
    holds 64 * 256 threads per cloud, so its loop repeats), random, with edge values in one coordinate.  z spreads the
    depths over both sides of the depth mask, and a few points sit at exactly its two limits."""
    rng = np.random.default_rng(seed + bins)
    half = (bins / 2) * (field / bins)
    edges = np.linspace(-half, half, bins + 1)
    e32 = edges.astype(F)
    vals = np.unique(np.concatenate([e32, np.nextafter(e32, F(-np.inf)), np.nextafter(e32, F(np.inf))]))
    outside = np.array([-1.5 * half, 1.5 * half, -3e4, 3e4], F)
    xs = np.concatenate([vals, outside])
    pairs = np.stack([np.repeat(xs, len(vals)), np.tile(vals, len(xs))], 1)
    pairs = np.concatenate([pairs, pairs[-4 * len(vals):, ::-1]])
    lo, hi = depth_limits(field, bins)
    on_limits = np.array([[lo, 0, 0], [0, -lo, 0], [hi, 0, 0], [0, 0, hi], [0, hi * 0.6, hi * 0.8]], F)

    def with_z(xy):
        z = rng.uniform(-0.4 * half, 0.4 * half, len(xy)) * (rng.random(len(xy)) < 0.7)
        return np.concatenate([xy, z[:, None], rng.random((len(xy), 1))], 1).astype(F)

    c1 = np.concatenate([with_z(pairs), np.concatenate([on_limits, np.zeros((len(on_limits), 1), F)], 1)])
    c2 = with_z(rng.uniform(-1.5 * half, 1.5 * half, (777, 2)))
    n3 = 64 * 256 * 2 + 1234
    xy3 = rng.uniform(-1.1 * half, 1.1 * half, (n3, 2))
    pick = rng.integers(0, len(vals), n3)
    xy3[::3, 0] = vals[pick[::3]]
    xy3[1::3, 1] = vals[pick[1::3]]
    c3 = with_z(xy3)
    return [np.zeros((0, 4), F), c1[rng.permutation(len(c1))], c2, c3]


def depth_limits(field, bins):
    half = (bins / 2) * (field / bins)
    return float(F(half * 0.25)), float(F(half * 1.0))          # both exact in fp32 for the fields used here


@pytest.mark.parametrize("field,bins", HIST_CASES)
def test_histogram_input_sits_on_every_edge(field, bins):
    clouds = hist_clouds(field, bins)
    assert len(clouds[0]) == 0 and len(clouds[3]) > 64 * 256 and all(c.dtype == F for c in clouds)
    half = (bins / 2) * (field / bins)
    edges = np.linspace(-half, half, bins + 1)
    c = clouds[1].astype(np.float64)
    for axis in (0, 1):
        for e in edges:
            e32 = float(F(e))
            at = c[:, axis] == e32
            below = c[:, axis] == float(np.nextafter(F(e), F(-np.inf)))
            above = c[:, axis] == float(np.nextafter(F(e), F(np.inf)))
            assert at.sum() >= bins and below.sum() >= bins and above.sum() >= bins
        assert (np.abs(c[:, axis]) > half).any()
    lo, hi = depth_limits(field, bins)
    assert F(lo) == lo and F(hi) == hi
    d = np.linalg.norm(clouds[1][:, :3], 2, axis=1)
    assert (d == F(lo)).sum() >= 2 and (d == F(hi)).sum() >= 3 and (d < lo).any() and (d > hi).any()
    h = om.point_cloud_to_histogram(field, bins, clouds[1])
    assert h.shape == (bins, bins) and (h > 0).all()
    assert om.point_cloud_to_histogram(field, bins, om.depth_mask(clouds[1], lo, hi)).sum() < h.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", (False, True), ids=("all", "masked"))
@pytest.mark.parametrize("field,bins", HIST_CASES)
def test_hip_histogram_bit_exact(field, bins, masked):
    from rangeldm_amd import metrics as M
    clouds = hist_clouds(field, bins)
    lo, hi = depth_limits(field, bins) if masked else (None, None)
    got = M.point_cloud_to_histogram(field, bins, [dev(c) for c in clouds], lo, hi)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, bins, bins)
    got = got.cpu().numpy()
    for i, c in enumerate(clouds):
        kept = om.depth_mask(c, lo, hi) if masked else c
        assert np.array_equal(got[i], om.point_cloud_to_histogram(field, bins, kept)), i
    assert got[0].sum() == 0
    # xyz-only clouds (stride 3) give the same counts
    got3 = M.point_cloud_to_histogram(field, bins, [dev(c[:, :3]) for c in clouds[1:3]], lo, hi).cpu().numpy()
    assert np.array_equal(got3, got[1:3])


# ---- spectral norm ---------------------------------------------------------------------------------------------------
SPECTRAL_BINS = (4, 8, 52, 104)


def spectral_sets(bins, seed=0):
    """x: 3 histograms, y: 5, integer counts with sums below 2^24.  Every histogram is noise plus its own block of a few
    rows and columns raised by its own amount, so that the leading singular value of every difference of pmfs stands clear
    of the second one.  y[2] is x[1]."""
    rng = np.random.default_rng(40 + bins + seed)
    out = []
    for i in range(8):
        h = rng.integers(0, 6, (bins, bins))
        rows = rng.permutation(bins)[:max(bins // 3, 1)]
        cols = rng.permutation(bins)[:max(bins // 3, 1)]
        h[np.ix_(rows, cols)] += 12 * (i + 2)
        out.append(h)
    x, y = np.stack(out[:3]).astype(np.int32), np.stack(out[3:]).astype(np.int32)
    y[2] = x[1]
    return x, y


@pytest.mark.parametrize("bins", SPECTRAL_BINS)
def test_spectral_inputs_have_a_clear_leading_singular_value(bins):
    x, y = spectral_sets(bins)
    assert x.shape == (3, bins, bins) and y.shape == (5, bins, bins)
    assert max(x.sum((1, 2)).max(), y.sum((1, 2)).max()) < 2 ** 24
    px = [h / h.sum() for h in x.astype(np.float64)]
    py = [h / h.sum() for h in y.astype(np.float64)]
    for i, a in enumerate(px):
        for j, b in enumerate(list(py) + list(px)):
            if (j == 2 and j < 5 and i == 1) or (j >= 5 and j - 5 == i):
                assert not (a - b).any()
                continue
            s = np.linalg.svd(a - b, compute_uv=False)
            assert s[1] / s[0] <= 0.99, (i, j, s[1] / s[0])
            assert abs(s[0] ** 2 - om.spectral_sq(x[i:i + 1], (list(y) + list(x))[j][None])[0, 0]) <= 1e-12 * s[0] ** 2


@pytest.mark.gpu
@pytest.mark.parametrize("bins", SPECTRAL_BINS)
def test_hip_spectral_sq_shapes(bins):
    from rangeldm_amd import metrics as M
    x, y = spectral_sets(bins)
    lam = M.spectral_sq(dev(x), dev(y))
    assert lam.dtype == torch.float32 and tuple(lam.shape) == (3, 5)
    lam = lam.cpu().numpy().astype(np.float64)
    ref = om.spectral_sq(x, y)
    assert lam[1, 2] == 0.0                                       # identical histograms: exactly 0
    rest = np.ones((3, 5), bool)
    rest[1, 2] = False
    assert np.abs(lam[rest] / ref[rest] - 1).max() < 1e-4
    assert tuple(M.spectral_sq(dev(y), dev(x)).shape) == (5, 3)
    assert np.abs(M.spectral_sq(dev(y), dev(x)).cpu().numpy().T[rest] / ref[rest] - 1).max() < 1e-4
    for h in (x, y):                                              # symmetric call
        sym = M.spectral_sq(dev(h)).cpu().numpy().astype(np.float64)
        ref_sym = om.spectral_sq(h, h)
        assert np.array_equal(sym, sym.T) and (np.diag(sym) == 0).all()
        off = ~np.eye(len(h), dtype=bool)
        assert np.abs(sym[off] / ref_sym[off] - 1).max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("bins", (6, 108))
def test_hip_spectral_sq_refuses_other_grids(bins):
    from rangeldm_amd import metrics as M
    h = dev(np.ones((2, bins, bins), np.int32))
    with pytest.raises(RuntimeError, match="multiple of 4, at most 104"):
        M.spectral_sq(h)
    with pytest.raises(RuntimeError, match="multiple of 4, at most 104"):
        M.compute_mmd(h, h)


# ---- JSD --------------------------------------------------------------------------------------------------------------
def jsd_fp64(hx, hy):
    """jsd.py:90-101 in numpy fp64 with scipy's rel_entr written out: x log(x / y) where x > 0, 0 where x = 0."""
    p = np.sum(np.asarray(hx, np.float64), axis=0).ravel()
    q = np.sum(np.asarray(hy, np.float64), axis=0).ravel()
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2

    def rel_entr(a):
        out = np.zeros_like(a)
        out[a > 0] = a[a > 0] * np.log(a[a > 0] / m[a > 0])
        return out
    return float(np.sqrt((rel_entr(p).sum() + rel_entr(q).sum()) / 2))


def jsd_sets(bins, seed=0):
    """name -> (hx, hy): sets of 1 and of 5 histograms, dense, with many empty bins, and with disjoint supports."""
    rng = np.random.default_rng(60 + bins + seed)
    dense = rng.integers(0, 2000, (6, bins, bins)).astype(np.int32)
    sparse = (rng.integers(0, 50, (6, bins, bins)) * (rng.random((6, bins, bins)) < 0.1)).astype(np.int32)
    sparse[:, 0, 0] += 1
    left = dense.copy()
    left[:, :, bins // 2:] = 0
    right = dense.copy()
    right[:, :, :bins // 2] = 0
    return {"dense 1 x 5": (dense[:1], dense[1:]), "dense 5 x 1": (dense[1:], dense[:1]), "dense 1 x 1": (dense[:1], dense[1:2]),
            "sparse 5 x 1": (sparse[:5], sparse[5:]), "sparse 1 x 1": (sparse[:1], sparse[1:2]),
            "mixed 5 x 5": (dense[:5], sparse[:5] + left[:5]), "disjoint 1 x 5": (left[:1], right[1:]),
            "disjoint 5 x 5": (left[:5], right[:5])}


@pytest.mark.parametrize("bins", (2, 104))
def test_jsd_statement_is_scipys(bins):
    for name, (hx, hy) in jsd_sets(bins).items():
        assert abs(jsd_fp64(hx, hy) - om.jsd(hx, hy)) < 1e-14, name
        if name.startswith("disjoint"):
            assert abs(jsd_fp64(hx, hy) - np.sqrt(np.log(2))) < 1e-14
        if name.startswith("sparse") and bins > 2:
            assert (hx.sum(0) == 0).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("bins", (2, 104))
def test_hip_jsd_shapes(bins):
    from rangeldm_amd import metrics as M
    for name, (hx, hy) in jsd_sets(bins).items():
        got = M.jsd_2d(dev(hx), dev(hy))
        assert abs(got - jsd_fp64(hx, hy)) < 1e-12, name
        if name.startswith("disjoint"):
            assert abs(got - np.sqrt(np.log(2))) < 1e-12
        assert M.jsd_2d(dev(hx), dev(hx)) == 0.0, name


# ---- MMD --------------------------------------------------------------------------------------------------------------
def mmd_sets(bins, seed=0):
    """x: 3 histograms, y: 5: counts of about 1000 per bin, each histogram with its own small deviation from its set's
    base, the two bases a little apart.  This is the regime of the metric (pmfs of sweeps of one scene type): every
    squared distance is below 5e-5, where the spectral kernel's 1e-4 relative is 1e-8 in a term exp(-2 lambda)."""
    rng = np.random.default_rng(80 + bins + seed)
    base_x = rng.integers(900, 1100, (bins, bins))
    base_y = base_x + rng.integers(-40, 41, (bins, bins)) + 30 * (np.arange(bins)[:, None] < bins // 2)
    x = np.stack([base_x + rng.integers(-10 * (i + 1), 10 * (i + 1) + 1, (bins, bins)) for i in range(3)])
    y = np.stack([base_y + rng.integers(-8 * (i + 1), 8 * (i + 1) + 1, (bins, bins)) for i in range(5)])
    return x.astype(np.int32), y.astype(np.int32)


@pytest.mark.parametrize("bins", (8, 52))
def test_mmd_inputs_are_in_the_metrics_regime(bins):
    x, y = mmd_sets(bins)
    assert x.shape == (3, bins, bins) and y.shape == (5, bins, bins) and x.min() > 0 and y.min() > 0
    lam = np.concatenate([om.spectral_sq(x, y).ravel(), om.spectral_sq(x, x).ravel(), om.spectral_sq(y, y).ravel()])
    assert lam.max() < 5e-5
    s1, s2, cross, mmd = om.compute_mmd(x, y)
    assert mmd > 0.2 * (1 - cross)                                # the combination does not cancel to nothing


@pytest.mark.gpu
@pytest.mark.parametrize("bins", (8, 52))
def test_hip_mmd_shapes(bins):
    from rangeldm_amd import metrics as M
    x, y = mmd_sets(bins)
    r = om.compute_mmd(x, y)
    s1, s2, cross, mmd = M.compute_mmd(dev(x), dev(y), return_terms=True)
    assert abs(s1 - r[0]) < 1e-8 and abs(s2 - r[1]) < 1e-8 and abs(cross - r[2]) < 1e-8
    assert abs(mmd / r[3] - 1) < 2e-4
    r = om.compute_mmd(y, x)
    s1, s2, cross, mmd = M.compute_mmd(dev(y), dev(x), return_terms=True)
    assert abs(s1 - r[0]) < 1e-8 and abs(s2 - r[1]) < 1e-8 and abs(cross - r[2]) < 1e-8
    assert abs(mmd / r[3] - 1) < 2e-4
    assert abs(M.compute_mmd(dev(x), dev(x))) < 1e-12
