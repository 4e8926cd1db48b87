"""Nearest neighbour with its index on the device (rangeldm_amd/csrc/nn_index.hip; metrics.nearest_neighbours and the F-score /
Hausdorff / density-aware CD read off it; `evaluate --match / --dcd-alpha`).

d^2, indices and hit counts are exact, so every case asks for EQUALITY with the numpy statement
metrics.nearest_neighbours_host (and, for d^2, with metrics.nearest_sq_dists).  The kernel has two ways out: a call with fewer
than 2 048 query blocks splits long target clouds over workgroups and merges the parts with a 64-bit atomicMin; a call with
2 048 query blocks or more streams every target cloud whole and writes directly.  `_embedded` puts the pairs under test
among 2 100 two-point filler pairs to reach the second, so each case runs both.

Shapes are the boundaries of the kernel: 256 lanes, 8 queries per lane (2 048 per workgroup), 512-point tiles, 64-point
sub-blocks.  Coordinates of the ragged calls are LiDAR-like (ranges 3-70 m); a target cloud is a subset / resampling of its
result cloud jittered by 5 cm, so thresholds of 0.05-0.5 m match some points and not others.
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

# together the twelve sizes {1, 3, 255, 256, 257, 511, 512, 513, 1025, 2047, 2048, 2049}, five pairs per call
SIZES = {(3, 3): [(1, 2049), (255, 513), (256, 2047), (257, 511), (2048, 1025)],
         (4, 5): [(3, 512), (2049, 1), (513, 256), (1025, 2048), (511, 257)]}
FILLERS = 2100          # two-point pairs: one query block each, so the call holds more than 2 048 query blocks
TAUS = [0.05, 0.1, 0.5]


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _lidar_like(rng, n, stride):
    r, az, el = rng.uniform(3.0, 70.0, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.43, 0.03, n)
    out = rng.standard_normal((n, stride))
    out[:, :3] = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el) + 1.7], 1)
    return out


def _ragged(strides):
    rng = np.random.default_rng(0)
    xs, ys = [], []
    for n, m in SIZES[strides]:
        x = _lidar_like(rng, n, strides[0])
        idx = rng.permutation(n)[:m] if m <= n else rng.integers(0, n, m)
        y = rng.standard_normal((m, strides[1]))
        y[:, :3] = x[idx, :3] + 0.05 * rng.standard_normal((m, 3))
        xs.append(x.astype(np.float32))
        ys.append(y.astype(np.float32))
    return xs, ys


@pytest.fixture(scope="module")
def ragged():
    """Per stride pair: the clouds and the host statement's six lists (computed once, never modified)."""
    out = {}
    for strides in SIZES:
        xs, ys = _ragged(strides)
        out[strides] = (xs, ys, M.nearest_neighbours_host(xs, ys, return_hits=True))
    return out


@pytest.fixture(scope="module")
def fillers():
    g = torch.Generator(device="cuda").manual_seed(7)
    fx = torch.rand((FILLERS, 2, 3), generator=g, device="cuda") * 10.0
    fy = torch.rand((FILLERS, 2, 3), generator=g, device="cuda") * 10.0
    return list(fx.unbind(0)), list(fy.unbind(0))


def _call(xs, ys):
    """nearest_neighbours with hits, as six lists of host arrays; dtypes checked on the way."""
    out = M.nearest_neighbours(xs, ys, return_hits=True)
    assert len(out) == 6 and all(len(part) == len(xs) for part in out)
    for part, dtype in zip(out, (torch.float32, torch.int64, torch.float32, torch.int64, torch.int32, torch.int32)):
        assert all(t.dtype == dtype and t.is_cuda and t.dim() == 1 for t in part)
    return [[t.cpu().numpy() for t in part] for part in out]


def _embedded(xs, ys, fillers, at=150):
    """The same call with the pairs under test placed from position `at` among the filler pairs; their six lists."""
    fx, fy = fillers
    out = _call(fx[:at] + list(xs) + fx[at:], fy[:at] + list(ys) + fy[at:])
    return [part[at:at + len(xs)] for part in out]


def _same(got, want):
    assert len(got) == len(want)
    for g_part, w_part in zip(got, want):
        assert len(g_part) == len(w_part)
        for g, w in zip(g_part, w_part):
            assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes()


@pytest.mark.parametrize("strides", list(SIZES))
def test_bit_equality(ragged, fillers, strides):
    xs, ys, want = ragged[strides]
    dx, dy = _dev(xs), _dev(ys)
    got = _call(dx, dy)
    _same(got, want)
    plain_x, plain_y = M.nearest_sq_dists(dx, dy)
    _same([got[0], got[2]], [[t.cpu().numpy() for t in plain_x], [t.cpu().numpy() for t in plain_y]])
    assert len(M.nearest_neighbours(dx, dy)) == 4
    for p, (n, m) in enumerate(SIZES[strides]):
        assert got[5][p].sum() == n and got[4][p].sum() == m
    _same(_embedded(dx, dy, fillers), want)              # every target cloud streamed whole: the direct way out
    # the fillers themselves, in the same call as host arrays
    fx, fy = fillers
    _same(_call(fx[:40], fy[:40]), M.nearest_neighbours_host([t.cpu().numpy() for t in fx[:40]], [t.cpu().numpy() for t in fy[:40]], True))


def test_tile_end_residues_agree_on_every_route(fillers):
    """The shared tile stage and sweep at the tile ends SIZES does not hold.  511, 512 and 513 are n mod 4 = 3, 0 and 1; here
    the targets are 509, 510, 514 and 515 points (1, 2, 2, 3, on both sides of the 512-point tile).  Alone the call splits
    514 and 515 into chunks of 257 and 258; among the fillers every cloud is streamed whole (a full tile, then 2 or 3 points).
    nearest_sq_dists, nearest_neighbours and knn_points(K=1) must give the host statement's d^2 bits in both directions, and
    the last two its indices."""
    rng = np.random.default_rng(9)
    xs = [_lidar_like(rng, n, 3).astype(np.float32) for n in (5, 2049, 257, 1)]
    ys = [_lidar_like(rng, m, 3).astype(np.float32) for m in (509, 510, 514, 515)]
    want = M.nearest_neighbours_host(xs, ys)
    fx, fy = fillers
    for at in (0, 150):                                  # alone; pairs 150 .. 153 of 2 104
        ax, ay = fx[:at] + _dev(xs) + (fx[at:] if at else []), fy[:at] + _dev(ys) + (fy[at:] if at else [])
        routes = (M.nearest_sq_dists(ax, ay), M.nearest_neighbours(ax, ay), M.knn_points(ax, ay, 1) + M.knn_points(ay, ax, 1))
        plain, index, knn = [[[t.cpu().numpy() for t in part[at:at + 4]] for part in route] for route in routes]
        knn = [[col[:, 0] for col in part] for part in knn]
        _same(plain, [want[0], want[2]])
        _same(index, want)
        _same(knn, want)
        _same([index[1], index[3]], [knn[1], knn[3]])


def test_ties_take_the_lowest_index(fillers):
    rng = np.random.default_rng(1)
    q = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    same = np.repeat(np.array([[1.5, -2.25, 0.5]], np.float32), 1030, 0)
    for got in (_call(_dev([q]), _dev([same])), _embedded(_dev([q]), _dev([same]), fillers)):
        assert (got[1][0] == 0).all() and got[5][0].tolist() == [300] + [0] * 1029
        assert (got[3][0] == M.nearest_neighbours_host(q, same)[3][0]).all()
    # 5 000 distinct grid points, one far point planted two or three times: across sub-blocks, tiles and chunks
    grid = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(13), indexing="ij"), -1).reshape(-1, 3)
    grid = grid[rng.permutation(len(grid))[:5000]].astype(np.float32)
    plant = np.array([100.0, 100.0, 100.0], np.float32)
    queries = np.stack([plant, plant, plant + np.float32(0.25), plant]).astype(np.float32)
    for spots, first in (((5, 517, 4100), 5), ((517, 4100), 517)):
        t = grid.copy()
        t[list(spots)] = plant
        want = M.nearest_neighbours_host(queries, t, return_hits=True)
        assert want[1][0].tolist() == [first] * 4
        for got in (_call(_dev([queries]), _dev([t])), _embedded(_dev([queries]), _dev([t]), fillers)):
            _same(got, want)
            assert got[5][0][first] == 4 and got[5][0].sum() == 4


def test_split_independence(fillers):
    rng = np.random.default_rng(2)
    x = _lidar_like(rng, 1, 3).astype(np.float32)
    y = _lidar_like(rng, 5000, 3).astype(np.float32)     # alone, the 5 000 targets are spread over ten workgroups
    want = M.nearest_neighbours_host(x, y, return_hits=True)
    alone = _call(_dev([x]), _dev([y]))
    _same(alone, want)
    fx, fy = fillers
    among_300 = _call(fx[:150] + _dev([x]) + fx[150:299], fy[:150] + _dev([y]) + fy[150:299])     # pair 150 of 300
    _same([part[150:151] for part in among_300], alone)
    _same(_embedded(_dev([x]), _dev([y]), fillers), alone)      # pair 150 of 2 101: the cloud is not split at all


def test_pairs_and_points_permuted(ragged):
    xs, ys, want = ragged[(4, 5)]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(xs)).tolist()
    got = _call(_dev([xs[i] for i in order]), _dev([ys[i] for i in order]))
    _same(got, [[part[i] for i in order] for part in want])
    p = 3                                                # (1025, 2048)
    sigma = rng.permutation(len(ys[p]))
    y_perm = ys[p][sigma]
    got = _call(_dev([xs[p]]), _dev([y_perm]))
    _same(got, M.nearest_neighbours_host(xs[p], y_perm, return_hits=True))
    assert got[0][0].tobytes() == want[0][p].tobytes()                                   # x -> y: d^2 unchanged
    assert got[2][0].tobytes() == want[2][p][sigma].tobytes()                            # y -> x: permuted with the points
    d = xs[p][:, None, :3] - y_perm[None, :, :3]
    d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]           # fp32, the kernel's expression
    rows = np.arange(len(xs[p]))
    assert (d[rows, got[1][0]] == got[0][0]).all() and (d.min(1) == got[0][0]).all()
    assert ((d == got[0][0][:, None]).argmax(1) == got[1][0]).all()                      # the lowest such index
    assert (got[5][0] == np.bincount(got[1][0], minlength=len(y_perm))).all()


def test_single_point_clouds(fillers):
    rng = np.random.default_rng(4)
    many = _lidar_like(rng, 2049, 4).astype(np.float32)
    one = _lidar_like(rng, 1, 3).astype(np.float32)
    for calls in ((lambda a, b: _call(_dev(a), _dev(b))), (lambda a, b: _embedded(_dev(a), _dev(b), fillers))):
        got = calls([many, one], [one, many])
        _same(got, M.nearest_neighbours_host([many, one], [one, many], return_hits=True))
        assert (got[1][0] == 0).all() and got[5][0].tolist() == [2049]
        assert (got[3][1] == 0).all() and got[4][1].tolist() == [2049]


@pytest.mark.parametrize("strides", list(SIZES))
def test_summaries_equal_host(ragged, strides):
    xs, ys, _ = ragged[strides]
    dx, dy = _dev(xs), _dev(ys)
    counts = M.match_counts(dx, dy, TAUS)
    assert counts.dtype == torch.int64 and counts.is_cuda and tuple(counts.shape) == (5, 3, 2)
    want = M.match_counts_host(xs, ys, TAUS)
    assert counts.cpu().numpy().tolist() == want.tolist()
    big = [p for p, (n, m) in enumerate(SIZES[strides]) if n > 200 and m > 200]
    assert all(0 < want[p, 0, 0] < want[p, 2, 0] for p in big)                          # not vacuous: tau separates points
    s, h = M.match_scores(dx, dy, TAUS), M.match_scores_host(xs, ys, TAUS)
    for k in ("precision", "recall", "fscore"):
        assert s[k].dtype == torch.float64 and s[k].cpu().numpy().tolist() == h[k].tolist()
    hd = M.hausdorff(dx, dy)
    assert hd.dtype == torch.float64 and hd.is_cuda and hd.cpu().numpy().tolist() == M.hausdorff_host(xs, ys).tolist()
    for alpha in (1.0, 50.0):
        # every term lies in [0, 1] and a mean has at most 2 049 of them: sums in two orders differ by less than
        # N * 2^-52 < 5e-13, exp differs by an ulp of a term; 1e-12 absolute holds for clouds of up to 5 000 points
        dcd = M.density_aware_chamfer(dx, dy, alpha)
        ref = M.density_aware_chamfer_host(xs, ys, alpha)
        assert dcd.dtype == torch.float64 and tuple(dcd.shape) == (5,)
        assert np.abs(dcd.cpu().numpy() - ref).max() <= 1e-12 and (ref > 0).all() and (ref < 1).all()
    both = M.pair_scores(dx, dy, taus=TAUS, alpha=50.0)
    xm, ym = M.chamfer_pairs(dx, dy)
    assert torch.equal(both["cd"], xm + ym) and torch.equal(both["match"]["counts"], counts)
    assert torch.equal(both["hausdorff"], hd) and torch.equal(both["dcd"], dcd)


def test_threshold_includes_equality_and_self_match():
    # integer points: every x is at distance exactly 2 or exactly 3 from the nearest y
    x = np.array([(0, 0, 0), (2, 3, 0), (10, 0, 2), (10, 0, -3)], np.float32)
    y = np.array([(2, 0, 0), (10, 0, 0)], np.float32)
    counts = M.match_counts(_dev([x]), _dev([y]), [2.0, 1.999, 3.0])
    assert counts.tolist() == [[[2, 2], [0, 0], [4, 2]]] == M.match_counts_host(x, y, [2.0, 1.999, 3.0]).tolist()
    rng = np.random.default_rng(5)
    c = _lidar_like(rng, 3000, 3).astype(np.float32)
    s = M.match_scores(_dev([c]), _dev([c]), 0.01)
    assert s["fscore"].tolist() == [[1.0]] and s["precision"].tolist() == [[1.0]]
    assert M.density_aware_chamfer(_dev([c]), _dev([c]), 50.0).tolist() == [0.0]
    assert M.hausdorff(_dev([c]), _dev([c])).tolist() == [[0.0, 0.0, 0.0]]


def test_transfer(ragged):
    xs, ys, want = ragged[(3, 3)]
    _, idx, _, _ = M.nearest_neighbours(_dev(xs), _dev(ys))
    rng = np.random.default_rng(6)
    values = [rng.integers(0, 20, (len(y), 2)) for y in ys]
    moved = M.transfer(_dev(values), idx)
    for p in range(len(xs)):
        assert tuple(moved[p].shape) == (len(xs[p]), 2)
        assert moved[p].cpu().numpy().tolist() == values[p][want[1][p]].tolist()


def test_cli_chamfer_match_dcd(tmp_path, capsys):
    rng = np.random.default_rng(8)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    xs, ys = [], []
    for i, (n, m) in enumerate([(900, 700), (1500, 1500), (64, 2000)]):
        x = _lidar_like(rng, n, 4).astype(np.float32)
        y = _lidar_like(rng, m, 4).astype(np.float32)
        k = min(n, m) // 2
        y[:k, :3] = x[:k, :3] + (0.2 * rng.standard_normal((k, 3))).astype(np.float32)
        x.tofile(a_dir / f"{i:03d}.bin")
        y.tofile(b_dir / f"{i:03d}.bin")
        xs.append(x)
        ys.append(y)
    argv = ["chamfer", str(a_dir), str(b_dir), "--match", "0.1", "0.5", "--dcd-alpha", "1"]
    res = E.main(argv)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == res and sorted(res) == ["cd", "dcd", "hausdorff", "match", "pairs", "task"]
    dx, dy = _dev(xs), _dev(ys)
    s = M.match_scores(dx, dy, [0.1, 0.5])
    match = res["match"]
    assert sorted(match) == ["fscore", "matched_result", "matched_target", "points_result", "points_target", "precision",
                             "recall", "tau"]
    assert match["tau"] == [0.1, 0.5]
    assert [match["matched_result"], match["matched_target"]] == s["counts"].sum(0).t().tolist()
    assert [match["points_result"], match["points_target"]] == [2464, 4200]
    assert 0 < match["matched_result"][0] < match["matched_result"][1] < 2464
    for k in ("precision", "recall", "fscore"):
        # the mean of three fp64 values in [0, 1]: two additions in whatever order, so two orders differ by at most 2^-51
        for t in range(2):
            assert abs(match[k][t] - math.fsum(s[k][:, t].tolist()) / 3) <= 2.0 ** -51
    hd = M.hausdorff(dx, dy)[:, 2].tolist()
    assert sorted(res["hausdorff"]) == ["max", "mean"] and res["hausdorff"]["max"] == max(hd)
    assert abs(res["hausdorff"]["mean"] - math.fsum(hd) / 3) <= 2.0 ** -51 * max(hd)       # (three values <= max(hd))
    dcd = M.density_aware_chamfer(dx, dy, 1.0).tolist()
    assert sorted(res["dcd"]) == ["alpha", "mean"] and res["dcd"]["alpha"] == 1.0
    assert abs(res["dcd"]["mean"] - math.fsum(dcd) / 3) <= 2.0 ** -51 and 0.0 < res["dcd"]["mean"] < 1.0
    # sharded over two ranks (no process group here: each call returns its own rank's sums): the integer totals add up
    a = E.build_parser().parse_args(argv)
    parts = [E.cmd_chamfer(a, rank, 2, torch.device("cuda"))["match"] for rank in (0, 1)]
    for key in ("matched_result", "matched_target"):
        assert [u + v for u, v in zip(parts[0][key], parts[1][key])] == match[key]
    assert parts[0]["points_result"] + parts[1]["points_result"] == 2464
    # without the flags: the keys of the parent commit, and the same cd
    plain = E.main(["chamfer", str(a_dir), str(b_dir)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(printed) == ["cd", "pairs", "task"] and printed == plain
    assert plain["cd"] == res["cd"]
    only_dcd = E.main(["chamfer", str(a_dir), str(b_dir), "--dcd-alpha", "1"])
    capsys.readouterr()
    assert sorted(only_dcd) == ["cd", "dcd", "pairs", "task"] and only_dcd["dcd"] == res["dcd"] and only_dcd["cd"] == plain["cd"]


def _check_blocks(block, taus, alpha):
    match, hd, dcd = block["match"], block["hausdorff"], block["dcd"]
    assert match["tau"] == taus and all(len(match[k]) == len(taus) for k in ("precision", "recall", "fscore"))
    for t in range(len(taus)):
        assert 0.0 <= match["precision"][t] <= 1.0 and 0.0 <= match["recall"][t] <= 1.0 and 0.0 <= match["fscore"][t] <= 1.0
        assert 0 <= match["matched_result"][t] <= match["points_result"] and 0 <= match["matched_target"][t] <= match["points_target"]
    assert match["matched_result"] == sorted(match["matched_result"])                    # more points match a larger tau
    assert 0.0 <= hd["mean"] <= hd["max"] and math.isfinite(hd["max"])
    assert dcd["alpha"] == alpha and 0.0 <= dcd["mean"] <= 1.0


def test_cli_vae_flags_keep_cd():
    plain = E.main(["vae", "--samples", "3", "--batch-size", "2"])
    res = E.main(["vae", "--samples", "3", "--batch-size", "2", "--match", "0.1", "1.0", "--dcd-alpha", "2"])
    assert sorted(res) == sorted(list(plain) + ["match", "hausdorff", "dcd"])
    assert all(res[k] == plain[k] for k in plain)                                        # cd included: the same bits
    _check_blocks(res, [0.1, 1.0], 2.0)


def test_cli_densification_flags_give_a_block_per_method(tmp_path):
    from rangeldm_amd import inference_conditional as IC
    exp = tmp_path / "exp"
    IC.main(["--cfg", "upsample", "--samples", "2", "--batch_size", "2", "--steps", "2", "--out", str(exp)])
    plain = E.main(["densification", "--exp", str(exp)])
    res = E.main(["densification", "--exp", str(exp), "--match", "0.1", "1.0", "--dcd-alpha", "2"])
    assert sorted(res) == sorted(list(plain) + ["match", "hausdorff", "dcd"])
    assert all(res[k] == plain[k] for k in plain)
    for m in ("ours", "nearest", "bicubic"):
        _check_blocks({k: res[k][m] for k in ("match", "hausdorff", "dcd")}, [0.1, 1.0], 2.0)
    # the three methods are scored against the same targets
    assert res["match"]["nearest"]["points_target"] == res["match"]["ours"]["points_target"]
