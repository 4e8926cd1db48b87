"""K nearest neighbours and what stands on them, on the device (rangeldm_amd/csrc/knn.hip; metrics.knn_points, self_neighbours,
estimate_normals, chamfer_distance with normals, plane_scores, statistical_outliers; `evaluate --normals K`).

d^2 and indices are exact, so every search case asks for EQUALITY of bytes with the numpy statement metrics.knn_points_host.
The kernel has three template instances (K <= 8: four queries per lane, K <= 16: two, K <= 32: one; 256 lanes, so query
blocks of 1 024, 512 and 256) and streams targets in tiles of 512; it has one route (a target cloud is never split).  Sizes sit
on both sides of every one of those boundaries and of K itself.  The host statement is computed once per stride pair at
K = 32; its first K columns are the statement at K (it sorts all candidates and cuts).

Normals are compared with metrics.estimate_normals_host ON THE DEVICE'S OWN INDICES, which the search cases pin.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import evaluate as E
from rangeldm_amd import metrics as M

pytestmark = pytest.mark.gpu

KS = [1, 3, 8, 9, 16, 17, 32]
# K - 1, K, K + 1 for every K above; wave, workgroup, tile (512) and two-tile boundaries; a long cloud
TARGETS = [1, 2, 3, 4, 7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
# the query blocks of the three instances (256, 512, 1 024) and a wave short of / past them
QUERIES = [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
STRIDES = [(3, 3), (4, 5)]
FILLERS = 2100


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _host(parts):
    return [t.cpu().numpy() for t in parts]


def _lidar_like(rng, n, stride):
    r, az, el = rng.uniform(3.0, 70.0, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.43, 0.03, n)
    out = rng.standard_normal((n, stride))
    out[:, :3] = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el) + 1.7], 1)
    return out.astype(np.float32)


def _same(got, want, K=None):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        w = w if K is None else w[:, :K]
        assert g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).astype(g.dtype).tobytes()


@pytest.fixture(scope="module")
def ragged():
    """Per stride pair: query clouds, target clouds and the host statement at K = 32, against the targets and of the targets
    against themselves with self excluded (computed once, never modified)."""
    out = {}
    for s, strides in enumerate(STRIDES):
        rng = np.random.default_rng(10 + s)
        ys = [_lidar_like(rng, m, strides[1]) for m in TARGETS]
        xs = []
        for p, m in enumerate(TARGETS):
            n = QUERIES[(p + 3 * s) % len(QUERIES)]
            x = _lidar_like(rng, n, strides[0])
            near = rng.random(n) < 0.5                   # half the queries sit 5 cm from a target, half anywhere
            x[near, :3] = ys[p][rng.integers(0, m, near.sum()), :3] + (0.05 * rng.standard_normal((near.sum(), 3))).astype(np.float32)
            xs.append(x)
        out[strides] = (xs, ys, M.knn_points_host(xs, ys, 32), M.knn_points_host(ys, ys, 32, exclude_self=True))
    return out


@pytest.fixture(scope="module")
def fillers():
    g = torch.Generator(device="cuda").manual_seed(7)
    fx = torch.rand((FILLERS, 2, 3), generator=g, device="cuda") * 10.0
    fy = torch.rand((FILLERS, 2, 3), generator=g, device="cuda") * 10.0
    return list(fx.unbind(0)), list(fy.unbind(0))


def _knn(xs, ys, K):
    d2, idx = M.knn_points(xs, ys, K)
    assert len(d2) == len(idx) == len(xs)
    assert all(t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == (len(x), K) for t, x in zip(d2, xs))
    assert all(t.dtype == torch.int64 and t.is_cuda and tuple(t.shape) == (len(x), K) for t, x in zip(idx, xs))
    return _host(d2), _host(idx)


def _self(xs, K):
    d2, idx = M.self_neighbours(xs, K)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (len(x), K) for t, x in zip(d2, xs))
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (len(x), K) for t, x in zip(idx, xs))
    return _host(d2), _host(idx)


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("K", KS)
def test_bit_equality(ragged, K, strides):
    xs, ys, want, want_self = ragged[strides]
    d2, idx = _knn(_dev(xs), _dev(ys), K)
    _same(d2, want[0], K)
    _same(idx, want[1], K)
    d2, idx = _self(_dev(ys), K)
    _same(d2, want_self[0], K)
    _same(idx, want_self[1], K)


@pytest.mark.parametrize("K", KS)
def test_short_clouds_end_in_empty_slots(ragged, K):
    xs, ys, _, _ = ragged[(3, 3)]
    short = [p for p, m in enumerate(TARGETS) if m <= K]
    assert short and TARGETS[0] == 1
    d2, idx = _knn(_dev([xs[p] for p in short]), _dev([ys[p] for p in short]), K)
    sd2, sidx = _self(_dev([ys[p] for p in short]), K)
    for k, p in enumerate(short):
        m = TARGETS[p]
        assert np.isinf(d2[k][:, m:]).all() and (d2[k][:, m:] > 0).all() and (idx[k][:, m:] == -1).all()
        assert np.isfinite(d2[k][:, :m]).all() and (np.sort(idx[k][:, :m], 1) == np.arange(m)).all()
        # against itself a point has m - 1 candidates: a one-point cloud has none
        assert np.isinf(sd2[k][:, m - 1:]).all() and (sidx[k][:, m - 1:] == -1).all() and (sidx[k][:, :m - 1] >= 0).all()
    assert sd2[0].shape == (1, K) and np.isinf(sd2[0]).all() and (sidx[0] == -1).all()


@pytest.mark.parametrize("K", KS)
def test_ties_take_the_lower_index(K):
    rng = np.random.default_rng(1)
    sites = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    c = sites[rng.integers(0, 64, 300)]                  # 300 points on 64 sites: every row is full of exact ties and zeros
    d2, idx = _knn(_dev([c]), _dev([c]), K)
    want = M.knn_points_host(c, c, K)
    _same(d2, want[0])
    _same(idx, want[1])
    assert (d2[0][:, 0] == 0).all()
    sd2, sidx = _self(_dev([c]), K)
    want = M.knn_points_host(c, c, K, exclude_self=True)
    _same(sd2, want[0])
    _same(sidx, want[1])
    assert not (sidx[0] == np.arange(300)[:, None]).any()
    same_site = (c[:, None, :] == c[None, :, :]).all(2)
    assert (same_site.sum(1) > 1).sum() > 250            # nearly every site holds several points
    for i in range(300):                                 # a row starts with the other points of its own site, in index order
        others = [j for j in same_site[i].nonzero()[0] if j != i][:K]
        assert sidx[0][i, :len(others)].tolist() == others and (sd2[0][i, :len(others)] == 0).all()
        assert len(others) == K or sd2[0][i, len(others)] > 0


@pytest.mark.parametrize("strides", STRIDES)
def test_k1_is_nearest_neighbours(ragged, strides):
    xs, ys, _, _ = ragged[strides]
    dx, dy = _dev(xs), _dev(ys)
    d2, idx = _knn(dx, dy, 1)
    xd, xi, _, _ = M.nearest_neighbours(dx, dy)
    _same([d[:, 0] for d in d2], _host(xd))
    _same([i[:, 0] for i in idx], _host(xi))


@pytest.mark.parametrize("K", [8, 16, 32])
def test_independent_of_the_rest_of_the_call(ragged, fillers, K):
    xs, ys, want, want_self = ragged[(4, 5)]
    pick = [0, 14, 21, 24, 27]                           # targets 1, 33, 511, 1023, 2049
    dx, dy = _dev([xs[p] for p in pick]), _dev([ys[p] for p in pick])
    fx, fy = fillers
    at = 150
    d2, idx = _knn(fx[:at] + dx + fx[at:], fy[:at] + dy + fy[at:], K)
    _same(d2[at:at + len(pick)], [want[0][p] for p in pick], K)
    _same(idx[at:at + len(pick)], [want[1][p] for p in pick], K)
    # the fillers themselves: two-point clouds, a row is both targets in order and then empty slots
    hd2, hidx = M.knn_points_host(_host(fx[:40]), _host(fy[:40]), K)
    _same(d2[:40], hd2)
    _same(idx[:40], hidx)
    sd2, sidx = _self(fy[:at] + dy + fy[at:], K)
    _same(sd2[at:at + len(pick)], [want_self[0][p] for p in pick], K)
    _same(sidx[at:at + len(pick)], [want_self[1][p] for p in pick], K)


def test_padded_tensors():
    rng = np.random.default_rng(2)
    lens_x, lens_y = [300, 1, 513], [77, 513, 2]
    x = torch.from_numpy(np.stack([_lidar_like(rng, 513, 4) for _ in range(3)])).cuda()
    y = torch.from_numpy(np.stack([_lidar_like(rng, 513, 4) for _ in range(3)])).cuda()
    xs, ys = [x[i, :n] for i, n in enumerate(lens_x)], [y[i, :n] for i, n in enumerate(lens_y)]
    for K in (3, 16):
        got = M.knn_points(x, y, K, x_lengths=torch.tensor(lens_x), y_lengths=lens_y)
        want = M.knn_points(xs, ys, K)
        for g, w in zip(got[0] + got[1], want[0] + want[1]):
            assert torch.equal(g, w)
        _same(_host(want[0]), M.knn_points_host(_host(xs), _host(ys), K)[0])
        got = M.self_neighbours(x, K, x_lengths=lens_x)
        want = M.self_neighbours(xs, K)
        for g, w in zip(got[0] + got[1], want[0] + want[1]):
            assert torch.equal(g, w)
    full = M.knn_points(x, y, 3)                         # no lengths: every row of the padded tensors
    assert [tuple(t.shape) for t in full[0]] == [(513, 3)] * 3
    n_list = M.estimate_normals(x, 8, x_lengths=lens_x)
    assert [tuple(t.shape) for t in n_list] == [(300, 3), (1, 3), (513, 3)] and (n_list[1] == 0).all()


def _scene(rng, n, lift=0):
    """A ground plane, a vertical wall and a tilted wall, each sampled uniformly over +- 20 m with 2 cm Gaussian noise along
    its own normal; the points are assigned to the three at random.  `lift` more points float 2 m above the ground."""
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
    if lift:
        out = np.concatenate([out, np.stack([rng.uniform(-20, 20, lift), rng.uniform(-20, 20, lift), np.full(lift, 0.3)], 1)])
    return out.astype(np.float32)


@pytest.mark.parametrize("n", [513, 2049])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_normals_equal_the_host_on_the_same_indices(K, n):
    """Both sides diagonalise the same fp64 covariance up to summation order (a relative 1e-15 or so); with a relative gap of
    at least 0.05 Davis-Kahan puts the eigenvectors within about 1e-13, so 1e-10 is asked of the vectors and 1e-12 of the
    trace of the eigenvalues.  Points whose two smallest eigenvalues are closer than that, or whose normal is perpendicular
    to the line of sight (the orientation is then decided by rounding), are left out; they must be at most 5 %.
    Measured on an MI355X over the six cases: at most 1.5e-15 on the vectors, 9.6e-16 of the trace, 0 to 0.19 % left out."""
    c = _scene(np.random.default_rng(0), n)
    dc = _dev([c])
    normals, lam = M.estimate_normals(dc, K, return_eigenvalues=True)
    assert normals[0].dtype == lam[0].dtype == torch.float64 and normals[0].is_cuda and tuple(normals[0].shape) == (n, 3)
    again = M.estimate_normals(dc, K)
    assert torch.equal(again[0], normals[0])
    _, idx = M.self_neighbours(dc, K)
    hn, hl = M.estimate_normals_host(c, [idx[0].cpu().numpy()], return_eigenvalues=True)
    got, got_l = normals[0].cpu().numpy(), lam[0].cpu().numpy()
    p64 = c.astype(np.float64)
    gap = (hl[0][:, 1] - hl[0][:, 0]) / hl[0][:, 2] >= 0.05
    sight = np.abs((hn[0] * p64).sum(1)) / np.linalg.norm(p64, axis=1) >= 1e-6
    keep = gap & sight
    print(f"K={K} n={n}: excluded {100 * (1 - keep.mean()):.2f} % (gap {100 * (1 - gap.mean()):.2f} %, sight {100 * (1 - sight.mean()):.2f} %), "
          f"max |dn| {np.abs(got - hn[0])[keep].max():.3e}, max |dlam| / trace {(np.abs(got_l - hl[0]).max(1) / hl[0].sum(1)).max():.3e}")
    assert (1 - keep.mean()) <= 0.05
    assert np.abs(got - hn[0])[keep].max() <= 1e-10
    assert (np.abs(got_l - hl[0]).max(1) <= 1e-12 * hl[0].sum(1)).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-14 and ((got * p64).sum(1) <= 0).all()
    assert (np.diff(got_l, axis=1) >= 0).all()


def test_normals_exact_and_degenerate():
    g = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(5, 12), indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([g, np.full((len(g), 1), 2)], 1).astype(np.float32)
    below = plane * np.float32([1, 1, -1])
    through = plane * np.float32([1, 1, 0])
    two = plane[:2]
    for K in (8, 16, 32):
        n, lam = M.estimate_normals(_dev([plane, below, through, two, plane[:1]]), K, return_eigenvalues=True)
        n, lam = _host(n), _host(lam)
        assert (n[0] == np.array([0.0, 0.0, -1.0])).all() and (lam[0][:, 0] == 0).all() and (lam[0][:, 1] > 0).all()
        assert (n[1] == np.array([0.0, 0.0, 1.0])).all()
        assert (n[2] == np.array([0.0, 0.0, 1.0])).all()                   # n . p == 0: the first non-zero component positive
        assert (np.signbit(n[0]) == (n[0] < 0)).all()                      # no negative zero leaves
        for k in (3, 4):                                 # two points, one point: no plane
            assert (n[k] == 0).all() and (lam[k] == 0).all()


@pytest.fixture(scope="module")
def scene_pairs():
    """Three jittered pairs of the scene and the host statement's plane scores at K = 8."""
    rng = np.random.default_rng(3)
    xs = [_scene(rng, n) for n in (700, 513, 300)]
    ys = []
    for x, m in zip(xs, (600, 513, 450)):
        pick = rng.permutation(len(x))[:m] if m <= len(x) else rng.integers(0, len(x), m)
        ys.append(x[pick] + (0.03 * rng.standard_normal((m, 3))).astype(np.float32))
    return xs, ys, M.plane_scores_host(xs, ys, 8)


def test_chamfer_distance_with_normals(scene_pairs):
    xs, ys, _ = scene_pairs
    dx, dy = _dev(xs), _dev(ys)
    plain, none = M.chamfer_distance(dx, dy, batch_reduction=None)
    assert none is None and plain.dtype == torch.float64                   # without normals: (dist, None), as before
    assert M.chamfer_distance(dx, dy)[1] is None
    xn, yn = M.estimate_normals(dx, 8), M.estimate_normals(dy, 8)
    want = M.normal_consistency_host(xs, ys, _host(xn), _host(yn))
    dist, ln = M.chamfer_distance(dx, dy, batch_reduction=None, x_normals=xn, y_normals=yn)
    assert torch.equal(dist, plain) and ln.dtype == torch.float64 and tuple(ln.shape) == (3,)
    assert (np.abs(ln.cpu().numpy() - want) <= 1e-12 * want).all() and (want > 0).all()
    # padded normals with padded clouds, and the reductions
    pad = lambda ts, w: torch.stack([torch.cat([t, t.new_zeros((700 - len(t), w))]) for t in ts])      # noqa: E731
    d2, l2 = M.chamfer_distance(pad(dx, 3), pad(dy, 3), [700, 513, 300], [600, 513, 450], batch_reduction=None,
                                x_normals=pad(xn, 3), y_normals=pad(yn, 3))
    assert torch.equal(d2, dist) and torch.equal(l2, ln)
    for red, f in (("mean", torch.mean), ("sum", torch.sum)):
        d3, l3 = M.chamfer_distance(dx, dy, batch_reduction=red, x_normals=xn, y_normals=yn)
        assert torch.equal(d3, f(dist)) and torch.equal(l3, f(ln))
    # a pair alone gives the bits it gives among the others
    alone = M.chamfer_distance(dx[1:2], dy[1:2], batch_reduction=None, x_normals=xn[1:2], y_normals=yn[1:2])
    assert torch.equal(alone[0], dist[1:2]) and torch.equal(alone[1], ln[1:2])


def test_plane_scores(scene_pairs):
    xs, ys, want = scene_pairs
    dx, dy = _dev(xs), _dev(ys)
    s = M.plane_scores(dx, dy, 8)
    assert sorted(s) == ["cd", "cd_plane", "normal_consistency"]
    assert all(v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (3,) for v in s.values())
    assert torch.equal(s["cd"], M.pair_scores(dx, dy)["cd"])
    for k in ("cd", "cd_plane", "normal_consistency"):
        rel = np.abs(s[k].cpu().numpy() - want[k]) / want[k]
        print(k, s[k].tolist(), want[k].tolist(), rel.max())
    for k in ("cd", "cd_plane", "normal_consistency"):
        assert (np.abs(s[k].cpu().numpy() - want[k]) <= 1e-12 * want[k]).all() and (want[k] > 0).all()
    assert (s["cd_plane"] <= s["cd"]).all()              # a component of a vector along a unit normal is no longer than it
    xn, yn = M.estimate_normals(dx, 8), M.estimate_normals(dy, 8)
    assert torch.equal(s["normal_consistency"], M.chamfer_distance(dx, dy, batch_reduction=None, x_normals=xn, y_normals=yn)[1])
    alone = M.plane_scores(dx[2:], dy[2:], 8)
    for k in s:
        assert torch.equal(alone[k], s[k][2:])


def test_statistical_outliers():
    c = _scene(np.random.default_rng(4), 1500, lift=20)
    for K, ratio in ((20, 2.0), (8, 1.0)):
        mask, mean, thr = M.statistical_outliers(_dev([c]), K, ratio, return_terms=True)
        assert mask[0].dtype == torch.bool and mask[0].is_cuda and tuple(mask[0].shape) == (1520,)
        assert torch.equal(M.statistical_outliers(_dev([c]), K, ratio)[0], mask[0])
        hmask, hmean, hthr = M.statistical_outliers_host(c, K, ratio, return_terms=True)
        close = np.abs(hmean[0] - hthr[0]) <= 1e-9 * hthr[0]               # such a point may fall on either side
        print(f"K={K}: {int(close.sum())} points within 1e-9 of the threshold, {int(hmask[0].sum())} outliers")
        assert close.sum() == 0
        assert (mask[0].cpu().numpy() == hmask[0])[~close].all()
        assert np.abs(mean[0].cpu().numpy() - hmean[0]).max() <= 1e-12 * hmean[0].max() and abs(float(thr[0]) - hthr[0]) <= 1e-12 * hthr[0]


def test_cli_chamfer_normals(tmp_path, capsys):
    rng = np.random.default_rng(5)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    xs, ys = [], []
    for i, (n, m) in enumerate([(900, 700), (600, 600), (257, 1000)]):
        x = np.concatenate([_scene(rng, n), rng.standard_normal((n, 1)).astype(np.float32)], 1)
        y = np.concatenate([_scene(rng, m), rng.standard_normal((m, 1)).astype(np.float32)], 1)
        x.tofile(a_dir / f"{i:03d}.bin")
        y.tofile(b_dir / f"{i:03d}.bin")
        xs.append(x)
        ys.append(y)
    argv = ["chamfer", str(a_dir), str(b_dir), "--normals", "8"]
    res = E.main(argv)
    first = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(first) == res and sorted(res) == ["cd", "pairs", "plane", "task"]
    assert sorted(res["plane"]) == ["cd_plane", "k", "normal_consistency"] and res["plane"]["k"] == 8
    s = M.plane_scores(_dev(xs), _dev(ys), 8)
    for k in ("cd_plane", "normal_consistency"):
        vals = s[k].tolist()
        # the mean of three positive fp64 values, added in whatever order: two orders differ by at most 2^-51 of the largest sum
        assert abs(res["plane"][k] - math.fsum(vals) / 3) <= 2.0 ** -51 * sum(vals) and res["plane"][k] > 0
    E.main(argv)
    assert capsys.readouterr().out.strip().splitlines()[-1] == first      # two runs: identical JSON
    # two ranks (no process group here: each call returns its own rank's sums over all pairs' count): the parts add up
    a = E.build_parser().parse_args(argv)
    parts = [E.cmd_chamfer(a, rank, 2, torch.device("cuda"))["plane"] for rank in (0, 1)]
    for k in ("cd_plane", "normal_consistency"):
        assert abs(parts[0][k] + parts[1][k] - res["plane"][k]) <= 2.0 ** -50 * res["plane"][k]
    plain = E.main(["chamfer", str(a_dir), str(b_dir)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(printed) == ["cd", "pairs", "task"] and printed == plain and plain["cd"] == res["cd"]
    both = E.main(argv + ["--match", "0.5", "--voxel", "0.2"])
    capsys.readouterr()
    assert both["plane"] == res["plane"] and both["cd"] == res["cd"]
    assert sorted(both) == ["cd", "hausdorff", "match", "occupancy", "pairs", "plane", "task", "voxel"]
