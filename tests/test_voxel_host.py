"""Voxel occupancy, host side (rangeldm_amd/metrics.py voxel_counts_host / voxel_scores_host; `evaluate --voxel`).

The numpy statement on a hand case whose voxels can be read off (0.1f / 0.1f is exactly 1; the fp32 denormal -1e-40 lands in
voxel -1), the argument errors that must be raised before a device is looked at, the out-of-range errors of the host
statement, and the four parsers that read --voxel.  No GPU.
"""
import numpy as np
import pytest
import torch

from rangeldm_amd import evaluate as E
from rangeldm_amd import metrics as M

HAND_X = np.array([(0, 0, 0), (.05, .05, .05), (.1, 0, 0), (-.01, 0, 0), (-1e-40, 0, 0)], np.float64)
HAND_Y = np.array([(.09, .09, .09), (.25, 0, 0)], np.float64)


def test_hand_case_counts_and_scores():
    # x: voxels (0,0,0) twice, (1,0,0), (-1,0,0) twice -> 3;  y: (0,0,0), (2,0,0) -> 2;  both: (0,0,0) -> 1
    v = np.float32(0.1)
    assert np.float32(0.1) / v == 1.0 and np.floor(np.float32(-1e-40) / v) == -1.0 and np.floor(np.float32(0.25) / v) == 2.0
    counts = M.voxel_counts_host([HAND_X], [HAND_Y], 0.1)
    assert counts.dtype == np.int64 and counts.tolist() == [[3, 2, 1]]
    assert M.voxel_counts_host(HAND_X, HAND_Y, 0.1).tolist() == [[3, 2, 1]]         # one array per side: one pair
    assert M.voxel_counts_host([HAND_X[::-1]], [HAND_Y[::-1]], 0.1).tolist() == [[3, 2, 1]]
    s = M.voxel_scores_host([HAND_X], [HAND_Y], 0.1)
    assert s["iou"].tolist() == [1 / 4] and s["precision"].tolist() == [1 / 3]
    assert s["recall"].tolist() == [1 / 2] and s["f1"].tolist() == [2 / 5]
    assert s["counts"].tolist() == [[3, 2, 1]]
    # wider points are read for xyz alone
    wide = np.concatenate([HAND_X, np.full((5, 2), 7.0)], 1)
    assert M.voxel_counts_host([wide], [HAND_Y], 0.1).tolist() == [[3, 2, 1]]


def test_argument_errors_need_no_gpu():
    good = torch.zeros((5, 3))
    for fn in (M.voxel_counts, M.voxel_scores):
        with pytest.raises(ValueError, match="empty"):
            fn([good, torch.zeros((0, 3))], [good, good])
        with pytest.raises(ValueError, match="2 x clouds against 3 y clouds"):
            fn([good, good], [good, good, good])
        for bad in (0, -1, float("nan"), float("inf"), 1e-50):
            with pytest.raises(ValueError, match="voxel"):
                fn([good], [good], voxel=bad)
        with pytest.raises(ValueError):
            fn([torch.zeros((5, 2))], [good])
        with pytest.raises(ValueError):
            fn([], [])
    g = np.zeros((5, 3))
    with pytest.raises(ValueError, match="empty"):
        M.voxel_counts_host([g, np.zeros((0, 3))], [g, g], 0.1)
    with pytest.raises(ValueError, match="2 x clouds against 3 y clouds"):
        M.voxel_counts_host([g, g], [g, g, g], 0.1)
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError, match="voxel"):
            M.voxel_counts_host([g], [g], bad)
    with pytest.raises(ValueError):
        M.voxel_counts_host([np.zeros((5, 2))], [g], 0.1)


@pytest.mark.parametrize("voxel", [0.1, 0.5, 1.0])
def test_host_refuses_points_out_of_range(voxel):
    g = np.zeros((4, 3), np.float32)
    nan = g.copy()
    nan[2, 1] = np.nan
    inf = g.copy()
    inf[0, 2] = -np.inf
    edge = g.copy()
    edge[3, 0] = np.float32(2.0 ** 20) * np.float32(voxel)
    for bad in (nan, inf, edge):
        with pytest.raises(ValueError, match="out of range"):
            M.voxel_counts_host([bad], [g], voxel)
        with pytest.raises(ValueError, match="out of range"):
            M.voxel_counts_host([g], [bad], voxel)
    # the lowest voxel index is in range: -2^20 itself
    low = g.copy()
    low[0, 0] = -np.float32(2.0 ** 20) * np.float32(voxel)
    assert np.floor(low[0, 0] / np.float32(voxel)) == -2.0 ** 20
    assert M.voxel_counts_host([low], [g], voxel).tolist() == [[2, 1, 1]]


def test_parsers_read_voxel():
    ap = E.build_parser()
    for argv in (["vae"], ["densification", "--exp", "e"], ["inpainting", "--exp", "e"], ["chamfer", "a", "b"]):
        assert ap.parse_args(argv).voxel is None
        assert ap.parse_args(argv + ["--voxel", "0.1"]).voxel == 0.1
    with pytest.raises(SystemExit):
        ap.parse_args(["generation", "a", "b", "--voxel", "0.1"])
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="voxel"):
            E.check_voxel_arg(ap.parse_args(["chamfer", "a", "b", "--voxel", str(bad)]))
    E.check_voxel_arg(ap.parse_args(["chamfer", "a", "b"]))


def test_occupancy_block_from_sums():
    block = E._occupancy_block([0.5, 1.0, 1.5, 0.25, 30.0, 20.0, 10.0], 2)
    assert block == {"iou": 0.25, "precision": 0.5, "recall": 0.75, "f1": 0.125,
                     "voxels_result": 30, "voxels_target": 20, "voxels_both": 10}
