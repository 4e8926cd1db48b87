"""The numpy statements of the K-nearest-neighbour metrics (metrics.knn_points_host, estimate_normals_host, plane_scores_host,
normal_consistency_host, statistical_outliers_host) and the argument checks, without a GPU.
"""
import numpy as np
import pytest
import torch

from rangeldm_amd import evaluate as E
from rangeldm_amd import metrics as M


def _double_loop(q, t, K, exclude_self):
    """Per query the (d2, index) pairs of all candidates, sorted as tuples, cut to K and padded with (+inf, -1)."""
    d2, idx = np.full((len(q), K), np.inf, np.float32), np.full((len(q), K), -1, np.int64)
    for i in range(len(q)):
        cand = []
        for j in range(len(t)):
            if exclude_self and i == j:
                continue
            dx, dy, dz = (np.float32(q[i, k]) - np.float32(t[j, k]) for k in range(3))
            cand.append((float(np.float32(np.float32(dx * dx + dy * dy) + dz * dz)), j))
        for s, (d, j) in enumerate(sorted(cand)[:K]):
            d2[i, s], idx[i, s] = d, j
    return d2, idx


@pytest.mark.parametrize("K", [1, 3, 8, 32])
def test_knn_points_host_against_a_double_loop(K):
    rng = np.random.default_rng(K)
    x = rng.standard_normal((23, 4)).astype(np.float32)
    y = rng.standard_normal((17, 3)).astype(np.float32)
    d2, idx = M.knn_points_host([x], [y], K)
    assert d2[0].dtype == np.float32 and idx[0].dtype == np.int64 and d2[0].shape == idx[0].shape == (23, K)
    want = _double_loop(x, y, K, False)
    assert d2[0].tobytes() == want[0].tobytes() and idx[0].tobytes() == want[1].tobytes()
    if K > 17:
        assert np.isinf(d2[0][:, 17:]).all() and (idx[0][:, 17:] == -1).all() and (idx[0][:, :17] >= 0).all()
    # an integer lattice drawn with repetition: rows full of exact ties and zeros, and the point itself left out
    c = rng.integers(0, 3, (40, 3)).astype(np.float32)
    for self_mode in (False, True):
        d2, idx = M.knn_points_host(c, c, K, exclude_self=self_mode)
        want = _double_loop(c, c, K, self_mode)
        assert d2[0].tobytes() == want[0].tobytes() and idx[0].tobytes() == want[1].tobytes()
    assert not (idx[0] == np.arange(40)[:, None]).any()                    # (self mode) no row holds its own index
    twin = [(c[:, None, :] == c[None, :, :]).all(2)[i].nonzero()[0] for i in range(40)]
    for i in range(40):
        others = [j for j in twin[i] if j != i][:K]
        assert idx[0][i, :len(others)].tolist() == others and (d2[0][i, :len(others)] == 0).all()


def test_knn_points_host_k1_is_nearest_neighbours_host():
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((n, 3)).astype(np.float32) for n in (1, 50)]
    ys = [rng.standard_normal((n, 3)).astype(np.float32) for n in (9, 1)]
    d2, idx = M.knn_points_host(xs, ys, 1)
    xd, xi, _, _ = M.nearest_neighbours_host(xs, ys)
    for p in range(2):
        assert d2[p][:, 0].tobytes() == xd[p].tobytes() and idx[p][:, 0].tobytes() == xi[p].tobytes()


def _lattice_plane():
    g = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(5, 12), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.full((len(g), 1), 2)], 1).astype(np.float32)


def test_normals_of_a_lattice_plane_are_exact():
    p = _lattice_plane()
    for K in (8, 16):
        _, idx = M.knn_points_host(p, p, K, exclude_self=True)
        normals, lam = M.estimate_normals_host(p, idx, return_eigenvalues=True)
        assert normals[0].dtype == np.float64 and normals[0].shape == (49, 3)
        assert (normals[0] == np.array([0.0, 0.0, -1.0])).all()           # towards the origin: the plane is above it
        assert (lam[0][:, 0] == 0.0).all() and (lam[0][:, 1] > 0.0).all()
    # below the sensor the normal points up; a cloud of two points has no plane
    q = p.copy()
    q[:, 2] = -2
    assert (M.estimate_normals_host(q, M.knn_points_host(q, q, 8, True)[1])[0] == np.array([0.0, 0.0, 1.0])).all()
    two = p[:2]
    n, lam = M.estimate_normals_host(two, M.knn_points_host(two, two, 8, True)[1], return_eigenvalues=True)
    assert (n[0] == 0).all() and (lam[0] == 0).all()
    # n . p == 0 (the plane through the origin): the first non-zero component is positive
    q[:, 2] = 0
    assert (M.estimate_normals_host(q, M.knn_points_host(q, q, 8, True)[1])[0] == np.array([0.0, 0.0, 1.0])).all()


def _scene(rng, n, jitter=0.0):
    """Ground plane, a vertical wall and a tilted wall, each sampled over +- 20 m with 2 cm noise along its own normal."""
    which = rng.integers(0, 3, n)
    u, v = rng.uniform(-20, 20, n), rng.uniform(-20, 20, n)
    frames = [((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1.7)),
              ((0, 1, 0), (0, 0, 1), (1, 0, 0), (25.0, 0, 0)),
              ((1, 0, 0), (0, 0.6, 0.8), (0, -0.8, 0.6), (0, 30.0, 5.0))]
    out = np.empty((n, 3))
    for k, (a, b, nrm, org) in enumerate(frames):
        m = which == k
        out[m] = (np.array(org) + u[m, None] * np.array(a) + v[m, None] * np.array(b)
                  + 0.02 * rng.standard_normal(m.sum())[:, None] * np.array(nrm))
    return (out + jitter * rng.standard_normal((n, 3))).astype(np.float32)


def test_plane_scores_host_against_a_restatement():
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    xs = [_scene(rng, n) for n in (300, 211)]
    ys = [x[rng.permutation(len(x))[:m]] + (0.03 * rng.standard_normal((m, 3))).astype(np.float32) for x, m in zip(xs, (250, 211))]
    K = 8
    s = M.plane_scores_host(xs, ys, K)
    assert sorted(s) == ["cd", "cd_plane", "normal_consistency"] and all(v.dtype == np.float64 and v.shape == (2,) for v in s.values())
    xd, xi, yd, yi = M.nearest_neighbours_host(xs, ys)
    for p in range(2):
        xn = M.estimate_normals_host(xs[p], M.knn_points_host(xs[p], xs[p], K, True)[1])[0]
        yn = M.estimate_normals_host(ys[p], M.knn_points_host(ys[p], ys[p], K, True)[1])[0]
        assert np.abs(np.linalg.norm(xn, axis=1) - 1).max() < 1e-14 and ((xn * xs[p]).sum(1) <= 0).all()
        x64, y64 = torch.from_numpy(xs[p]).double(), torch.from_numpy(ys[p]).double()
        tx, ty = torch.from_numpy(xn), torch.from_numpy(yn)
        i, j = torch.from_numpy(xi[p]), torch.from_numpy(yi[p])
        nc = (1 - F.cosine_similarity(tx, ty[i], dim=1, eps=1e-6).abs()).mean() + (1 - F.cosine_similarity(ty, tx[j], dim=1, eps=1e-6).abs()).mean()
        plane = (((x64 - y64[i]) * ty[i]).sum(1) ** 2).mean() + (((y64 - x64[j]) * tx[j]).sum(1) ** 2).mean()
        cd = xd[p].astype(np.float64).mean() + yd[p].astype(np.float64).mean()
        assert abs(s["normal_consistency"][p] - float(nc)) <= 1e-12 * float(nc)
        assert abs(s["cd_plane"][p] - float(plane)) <= 1e-12 * float(plane)
        assert abs(s["cd"][p] - cd) <= 1e-12 * cd
        assert abs(M.normal_consistency_host([xs[p]], [ys[p]], [xn], [yn])[0] - float(nc)) <= 1e-12 * float(nc)
        # a component of a vector along a unit normal is no longer than the vector
        assert 0 < s["cd_plane"][p] <= s["cd"][p] and 0 <= s["normal_consistency"][p] <= 2
    # zero normals (a point without a plane) meet the eps of cosine_similarity: the term is 1, on both sides of the statement
    zero = [np.zeros((3, 3))]
    unit = [np.tile(np.array([[0.0, 0.0, 1.0]]), (3, 1))]
    c = [np.eye(3, dtype=np.float32)]
    assert M.normal_consistency_host(c, c, zero, unit).tolist() == [2.0]


def test_statistical_outliers_host_against_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(2)
    cloud = np.concatenate([_scene(rng, 600), rng.uniform(-20, 20, (12, 3)).astype(np.float32) + np.float32([0, 0, 12])])
    K, ratio = 6, 2.0
    mask, mean, thr = M.statistical_outliers_host(cloud, K, ratio, return_terms=True)
    assert mask[0].dtype == np.bool_ and mask[0].shape == (612,)
    dist, _ = cKDTree(cloud.astype(np.float64)).query(cloud.astype(np.float64), k=K + 1)
    ref = dist[:, 1:].mean(1)                            # column 0 is the point itself
    # the tree works on fp64 coordinates, the statement on fp32 d^2: a relative 1e-6 of a distance
    assert np.abs(mean[0] - ref).max() <= 1e-5 * ref.max()
    ref_thr = ref.mean() + ratio * ref.std()
    near = np.abs(ref - ref_thr) <= 1e-4 * ref_thr
    assert ((ref > ref_thr) == mask[0])[~near].all() and near.sum() <= 2
    assert mask[0][600:].sum() >= 10 and mask[0][:600].sum() <= 30       # the floating points are found, the scene is kept
    # a one-point cloud has no neighbour and is no outlier
    assert M.statistical_outliers_host(cloud[:1], 4)[0].tolist() == [False]


@pytest.mark.parametrize("K", [0, 33, -1, 2.0, "8", None, True])
def test_bad_k_raises_before_a_kernel_runs(K):
    c = [torch.zeros((4, 3))]                            # CPU tensors: K is refused before the device is asked for
    h = [np.zeros((4, 3), np.float32)]
    for fn in (lambda: M.knn_points(c, c, K), lambda: M.self_neighbours(c, K), lambda: M.estimate_normals(c, K),
               lambda: M.plane_scores(c, c, K), lambda: M.statistical_outliers(c, K), lambda: M.knn_points_host(h, h, K),
               lambda: M.plane_scores_host(h, h, K), lambda: M.statistical_outliers_host(h, K)):
        with pytest.raises(ValueError, match="K must be"):
            fn()


def test_bad_shapes_raise():
    c = [torch.zeros((4, 3))]
    for fn in (lambda: M.knn_points([torch.zeros((0, 3))], c, 3), lambda: M.knn_points(c + c, c, 3), lambda: M.self_neighbours([], 3),
               lambda: M.plane_scores(c, c + c, 3), lambda: M.estimate_normals(torch.zeros((2, 4, 2)), 3),
               lambda: M.statistical_outliers(c, 3, float("nan")), lambda: M.statistical_outliers_host([np.zeros((4, 3))], 3, "x"),
               lambda: M.chamfer_distance(c, c, x_normals=c), lambda: M.chamfer_distance(c, c, y_normals=c),
               lambda: M.chamfer_distance(c, c, x_normals=[torch.zeros((5, 3))], y_normals=c),
               lambda: M.chamfer_distance(c, c, x_normals=torch.zeros((1, 3, 3)), y_normals=c),
               lambda: M.chamfer_distance(c, c, x_normals=c + c, y_normals=c),
               lambda: M.knn_points_host([np.zeros((4, 3))] * 2, [np.zeros((4, 3))], 3),
               lambda: M.knn_points_host([np.zeros((4, 3))], [np.zeros((5, 3))], 3, exclude_self=True),
               lambda: M.estimate_normals_host([np.zeros((4, 3))], [np.zeros((5, 2), np.int64)])):
        with pytest.raises(ValueError):
            fn()


def test_cpu_tensors_are_refused():
    c = [torch.zeros((4, 3))]
    for fn in (lambda: M.knn_points(c, c, 3), lambda: M.self_neighbours(c, 3), lambda: M.estimate_normals(c, 3),
               lambda: M.statistical_outliers(c, 3), lambda: M.chamfer_distance(c, c, x_normals=c, y_normals=c)):
        with pytest.raises(RuntimeError):
            fn()


def test_parsers_accept_normals():
    ap = E.build_parser()
    for argv in (["vae"], ["densification", "--exp", "e"], ["inpainting", "--exp", "e"], ["chamfer", "a", "b"]):
        assert ap.parse_args(argv).normals is None
        E.check_normals_arg(ap.parse_args(argv))
        a = ap.parse_args(argv + ["--normals", "8"])
        assert a.normals == 8
        E.check_normals_arg(a)
        for bad in ("0", "33", "-4"):
            with pytest.raises(ValueError):
                E.check_normals_arg(ap.parse_args(argv + ["--normals", bad]))
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--normals", "8.5"])
    with pytest.raises(SystemExit):
        ap.parse_args(["generation", "g", "r", "--normals", "8"])
    # refused before a file is read: the folders do not exist
    with pytest.raises(ValueError, match="K must be"):
        E.cmd_chamfer(ap.parse_args(["chamfer", "/nonexistent/a", "/nonexistent/b", "--normals", "40"]), 0, 1, None)
