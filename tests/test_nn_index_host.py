"""The numpy statements of the nearest-neighbour metrics (metrics.nearest_neighbours_host and what is read off it) and the
argument checks, without a GPU.

Hand case, worked on paper.  X = (0,0,0), (1,0,0), (0,2,0), (4,0,0);  Y = (0,0,0), (2,0,0), (0,1,0).

    X -> Y   d^2 = 0, 1, 1, 4     idx = 0, 0, 2, 1     (x1 is at d^2 = 1 from y0 AND y1: the lower index)
    Y -> X   d^2 = 0, 1, 1        idx = 0, 1, 0        (y1 is at 1 from x1, at 4 from x0 and x3; y2 at 1 from x0 AND x2)
    y_hits = 2, 1, 1              x_hits = 2, 1, 0, 0
    tau 0.5: 1 of 4 and 1 of 3 matched -> p = 1/4, r = 1/3, f = 2/7;   tau 1: 3 of 4 and 3 of 3 -> p = 3/4, r = 1, f = 6/7
    Hausdorff  X -> Y = 2,  Y -> X = 1,  symmetric = 2
    DCD, alpha = ln 2 (exp(-alpha d^2) = 2^-d^2):  X terms 1 - 1/2, 1 - (1/2)/2, 1 - 1/2, 1 - 1/16 -> mean 2.6875 / 4;
         Y terms 1 - 1/2, 1 - 1/2, 1 - (1/2)/2 -> mean 1.75 / 3;  dcd = (2.6875 / 4 + 1.75 / 3) / 2
"""
import math

import numpy as np
import pytest

from rangeldm_amd import evaluate as E
from rangeldm_amd import metrics as M

HAND_X = np.array([(0, 0, 0), (1, 0, 0), (0, 2, 0), (4, 0, 0)], np.float32)
HAND_Y = np.array([(0, 0, 0), (2, 0, 0), (0, 1, 0)], np.float32)


def test_hand_case():
    xd, xi, yd, yi, xh, yh = M.nearest_neighbours_host(HAND_X, HAND_Y, return_hits=True)
    assert len(xd) == 1 and xd[0].dtype == np.float32 and xi[0].dtype == np.int64 and xh[0].dtype == np.int32
    assert xd[0].tolist() == [0, 1, 1, 4] and xi[0].tolist() == [0, 0, 2, 1]
    assert yd[0].tolist() == [0, 1, 1] and yi[0].tolist() == [0, 1, 0]
    assert yh[0].tolist() == [2, 1, 1] and xh[0].tolist() == [2, 1, 0, 0]
    assert len(M.nearest_neighbours_host(HAND_X, HAND_Y)) == 4
    counts = M.match_counts_host([HAND_X], [HAND_Y], [0.5, 1.0])
    assert counts.dtype == np.int64 and counts.tolist() == [[[1, 1], [3, 3]]]
    s = M.match_scores_host([HAND_X], [HAND_Y], [0.5, 1.0])
    assert s["precision"].tolist() == [[1 / 4, 3 / 4]] and s["recall"].tolist() == [[1 / 3, 1.0]]
    assert s["fscore"].tolist() == [[2 * (1 / 4) * (1 / 3) / (1 / 4 + 1 / 3), 2 * (3 / 4) / (3 / 4 + 1.0)]]
    assert abs(s["fscore"][0, 0] - 2 / 7) < 1e-15 and abs(s["fscore"][0, 1] - 6 / 7) < 1e-15
    assert s["points"].tolist() == [[4, 3]] and s["tau"] == [0.5, 1.0]
    assert M.hausdorff_host(HAND_X, HAND_Y).tolist() == [[2.0, 1.0, 2.0]]
    dcd = M.density_aware_chamfer_host(HAND_X, HAND_Y, math.log(2.0))
    assert dcd.shape == (1,) and abs(dcd[0] - (2.6875 / 4 + 1.75 / 3) / 2) < 1e-15


def test_double_loop_with_a_tie():
    rng = np.random.default_rng(2)
    x = rng.integers(-3, 4, (7, 4)).astype(np.float32)
    y = rng.integers(-3, 4, (5, 3)).astype(np.float32)
    y[3] = y[1]                                          # an exact tie for every query whose neighbour is y1
    x[0, :3] = y[1]
    xd, xi, yd, yi = M.nearest_neighbours_host([x], [y])
    for q, t, d2, idx in ((x, y, xd[0], xi[0]), (y, x, yd[0], yi[0])):
        for i in range(len(q)):
            best, arg = None, None
            for j in range(len(t)):
                dx, dy, dz = (np.float32(q[i, k]) - np.float32(t[j, k]) for k in range(3))
                d = np.float32(np.float32(dx * dx + dy * dy) + dz * dz)
                if best is None or d < best:             # strict: the first minimum is kept
                    best, arg = d, j
            assert d2[i] == best and idx[i] == arg
    assert xd[0][0] == 0 and xi[0][0] == 1               # y1 and y3 coincide: the lower index


def test_d2_agrees_with_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    x = rng.integers(-64, 65, (700, 3)).astype(np.float32)
    y = rng.integers(-64, 65, (450, 3)).astype(np.float32)
    xd, xi, yd, yi = M.nearest_neighbours_host([x], [y])
    for q, t, d2, idx in ((x, y, xd[0], xi[0]), (y, x, yd[0], yi[0])):
        dist, _ = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
        # integers with |c| <= 64: d^2 <= 3 * 128^2 is exact in fp32 and fp64; the tree returns sqrt(d^2), correctly rounded
        assert (np.sqrt(d2.astype(np.float64)) == dist).all()
        assert (((q - t[idx]) ** 2).sum(1) == d2).all()


def test_hits_sum_to_the_other_cloud():
    rng = np.random.default_rng(4)
    xs = [rng.standard_normal((n, 3)).astype(np.float32) for n in (1, 40, 333)]
    ys = [rng.standard_normal((n, 3)).astype(np.float32) for n in (17, 1, 200)]
    _, xi, _, yi, xh, yh = M.nearest_neighbours_host(xs, ys, return_hits=True)
    for p in range(3):
        assert len(xh[p]) == len(xs[p]) and len(yh[p]) == len(ys[p])
        assert yh[p].sum() == len(xs[p]) and xh[p].sum() == len(ys[p])
        assert (yh[p] == np.bincount(xi[p], minlength=len(ys[p]))).all()


def test_fscore_is_zero_when_nothing_matches():
    x = np.zeros((5, 3), np.float32)
    y = np.full((4, 3), 10.0, np.float32)
    s = M.match_scores_host(x, y, [0.1, 1.0])
    assert s["counts"].tolist() == [[[0, 0], [0, 0]]]
    assert s["precision"].tolist() == [[0.0, 0.0]] and s["recall"].tolist() == [[0.0, 0.0]] and s["fscore"].tolist() == [[0.0, 0.0]]
    # a cloud against itself: everything matches, no density penalty
    s = M.match_scores_host(HAND_X, HAND_X, 0.01)
    assert s["fscore"].tolist() == [[1.0]] and M.density_aware_chamfer_host(HAND_X, HAND_X, 3.0).tolist() == [0.0]


@pytest.mark.parametrize("tau", [0.0, -0.1, float("nan"), float("inf"), [0.1, 0.0], []])
def test_bad_tau_raises(tau):
    for fn in (M.match_counts_host, M.match_scores_host, M.match_counts, M.match_scores):
        with pytest.raises(ValueError):
            fn([HAND_X], [HAND_Y], tau)


def test_bad_alpha_raises():
    for fn in (M.density_aware_chamfer_host, M.density_aware_chamfer):
        with pytest.raises(ValueError, match="alpha is required"):
            fn([HAND_X], [HAND_Y])
        for alpha in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn([HAND_X], [HAND_Y], alpha)
    with pytest.raises(ValueError):
        M.nearest_neighbours_host([HAND_X, HAND_X], [HAND_Y])


def test_parsers_accept_the_flags():
    ap = E.build_parser()
    for argv in (["vae"], ["densification", "--exp", "e"], ["inpainting", "--exp", "e"], ["chamfer", "a", "b"]):
        a = ap.parse_args(argv)
        assert a.match is None and a.dcd_alpha is None and a.voxel is None
        a = ap.parse_args(argv + ["--match", "0.1", "0.5", "--dcd-alpha", "50"])
        assert a.match == [0.1, 0.5] and a.dcd_alpha == 50.0
        E.check_nn_args(a)
        assert E._nn_len(a) == 14
        for bad in (["--match", "0"], ["--dcd-alpha", "-1"], ["--match", "0.1", "nan"]):
            with pytest.raises(ValueError):
                E.check_nn_args(ap.parse_args(argv + bad))
    with pytest.raises(SystemExit):
        ap.parse_args(["generation", "g", "r", "--match", "0.1"])
