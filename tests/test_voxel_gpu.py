"""Voxel occupancy on the device (rangeldm_amd/csrc/voxel.hip; metrics.voxel_counts / voxel_scores; `evaluate --voxel`).

The counts are integers, so every case asks for EQUALITY with the numpy statement metrics.voxel_counts_host: the hand case, a
ragged call (sizes 1 .. 4 097, strides 3 / 4 / 5, two voxel sizes), integer-valued clouds with many duplicates, a pair of
5 000 copies of one point, coordinates one ulp either side of a voxel boundary, two pairs that share coordinates across
sides, permutations of points and of pairs, a call of more than 2^24 points (more than one chunk of hash tables), the
out-of-range errors and the call after them, and the command line.

Ragged call: coordinates are N(0, diag(20, 20, 1)^2) metres (standard deviations 20, 20, 1), y a copy of part of x jittered
with sigma = 0.05 (drawn with replacement where y is the longer side).  With default_rng(0) the host statement gives the
(4097, 3001) pair c = 689 at voxel 0.1 and 2 363 at 0.5 for strides (3, 3), and 707 and 2 322 for strides (4, 5); the test
asserts 0 < c < min(a, b) for every pair with more than one point per side (a one-point side cannot satisfy it).
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

HAND_X = np.array([(0, 0, 0), (.05, .05, .05), (.1, 0, 0), (-.01, 0, 0), (-1e-40, 0, 0)], np.float64)     # tests/test_voxel_host.py
HAND_Y = np.array([(.09, .09, .09), (.25, 0, 0)], np.float64)
SIZES = [(1, 1), (1, 777), (777, 1), (2049, 513), (4097, 3001), (2048, 2048), (2048, 2049)]


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _equal_host(xs, ys, voxel):
    got = M.voxel_counts(_dev(xs), _dev(ys), voxel)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(xs), 3)
    want = M.voxel_counts_host(xs, ys, voxel)
    assert got.cpu().numpy().tolist() == want.tolist()
    return want


def _ragged(xs_stride, ys_stride):
    rng = np.random.default_rng(0)
    std = np.array([20.0, 20.0, 1.0])
    xs, ys = [], []
    for n, m in SIZES:
        x = rng.standard_normal((n, xs_stride))
        x[:, :3] *= std
        idx = rng.permutation(n)[:m] if m <= n else rng.integers(0, n, m)
        y = rng.standard_normal((m, ys_stride))
        y[:, :3] = x[idx, :3] + 0.05 * rng.standard_normal((m, 3))
        xs.append(x.astype(np.float32))
        ys.append(y.astype(np.float32))
    return xs, ys


@pytest.fixture(scope="module")
def ragged():
    return {strides: _ragged(*strides) for strides in ((3, 3), (4, 5))}


def test_hand_case():
    xs, ys = [HAND_X.astype(np.float32)], [HAND_Y.astype(np.float32)]
    assert _equal_host(xs, ys, 0.1).tolist() == [[3, 2, 1]]
    s = M.voxel_scores(_dev(xs), _dev(ys), 0.1)
    assert all(s[k].dtype == torch.float64 and s[k].is_cuda and tuple(s[k].shape) == (1,) for k in M.VOXEL_SCORES)
    assert [float(s[k]) for k in M.VOXEL_SCORES] == [1 / 4, 1 / 3, 1 / 2, 2 / 5]
    assert s["counts"].tolist() == [[3, 2, 1]]
    # fp64 inputs are rounded to fp32 like the host statement's astype (the denormal point left out: that conversion is
    # torch's, not this library's); a padded tensor with lengths is taken too
    assert M.voxel_counts(_dev([HAND_X[:4]]), _dev([HAND_Y]), 0.1).tolist() == [[3, 2, 1]]
    pad_x = torch.zeros((1, 8, 3)).cuda()
    pad_x[0, :5] = torch.from_numpy(HAND_X).float()
    pad_x[0, 5:] = 50.0
    pad_y = torch.from_numpy(HAND_Y).float().cuda()[None]
    assert M.voxel_counts(pad_x, pad_y, 0.1, x_lengths=torch.tensor([5])).tolist() == [[3, 2, 1]]


@pytest.mark.parametrize("voxel", [0.1, 0.5])
@pytest.mark.parametrize("strides", [(3, 3), (4, 5)])
def test_ragged_call_equals_host(ragged, strides, voxel):
    xs, ys = ragged[strides]
    want = _equal_host(xs, ys, voxel)
    for (n, m), (a, b, c) in zip(SIZES, want.tolist()):
        assert 1 <= a <= n and 1 <= b <= m
        if n > 1 and m > 1:
            assert 0 < c < min(a, b), (n, m, a, b, c)        # the case is not vacuous: some voxels shared, not all
    s = M.voxel_scores(_dev(xs), _dev(ys), voxel)
    h = M.voxel_scores_host(xs, ys, voxel)
    for k in M.VOXEL_SCORES:
        assert s[k].cpu().numpy().tolist() == h[k].tolist()


@pytest.mark.parametrize("voxel", [1.0, 0.5])
def test_integer_valued_clouds(voxel):
    rng = np.random.default_rng(5)
    xs = [rng.integers(-8, 8, (n, 3)).astype(np.float32) for n in (1000, 2500, 7, 6000)]
    ys = [rng.integers(-8, 8, (n, 3)).astype(np.float32) for n in (1300, 9, 4100, 6000)]
    want = _equal_host(xs, ys, voxel)
    # exact arithmetic: the voxels are the distinct integer points themselves (at 0.5, twice them)
    for x, y, row in zip(xs, ys, want.tolist()):
        sx, sy = {tuple(p) for p in x.tolist()}, {tuple(p) for p in y.tolist()}
        assert row == [len(sx), len(sy), len(sx & sy)]
    assert want[3, 0] > 3000 and want[3, 0] < 4096             # many duplicates: 6 000 points in 4 096 cells


def test_duplicate_pair():
    p = np.array([[12.34, -5.6, 0.78]], np.float32)
    assert _equal_host([np.repeat(p, 5000, 0)], [np.repeat(p, 5000, 0)], 0.1).tolist() == [[1, 1, 1]]


def test_boundaries_one_ulp_apart():
    on = np.arange(-5, 6).astype(np.float32) * np.float32(0.5)
    below = np.nextafter(on, np.float32(-np.inf))
    assert (np.floor(on / np.float32(0.5)) - np.floor(below / np.float32(0.5)) == 1.0).all()     # as numpy says
    x = np.zeros((22, 3), np.float32)
    x[:, 0] = np.concatenate([on, below])
    for axis in range(3):
        xs = [np.roll(x, axis, 1)]
        # targets: the boundary values alone / the values one ulp below alone
        y_on, y_below = np.roll(x[:11], axis, 1), np.roll(x[11:], axis, 1)
        assert _equal_host(xs, [y_on], 0.5).tolist() == [[12, 11, 11]]
        assert _equal_host(xs, [y_below], 0.5).tolist() == [[12, 11, 11]]
        assert _equal_host([y_on[-1:]], [y_below[-1:]], 0.5).tolist() == [[1, 1, 0]]
    # fp32 denormals are kept: -1e-40 is in voxel -1, +1e-40 in voxel 0
    tiny = np.array([[-1e-40, 1e-40, 0.0]], np.float32)
    zero = np.zeros((1, 3), np.float32)
    assert _equal_host([tiny], [zero], 0.1).tolist() == [[1, 1, 0]]


def test_pairs_are_isolated():
    rng = np.random.default_rng(9)
    shared = (rng.standard_normal((3000, 3)) * 5.0).astype(np.float32)
    far_a = shared + np.float32(500.0)
    far_b = shared - np.float32(500.0)
    # pair 0: x = shared, y far away;  pair 1: x far away (elsewhere), y = shared
    want = _equal_host([shared, far_a], [far_b, shared], 0.5)
    assert want[0, 2] == 0 and want[1, 2] == 0
    assert want[0, 0] == want[1, 1] > 1000


def test_order_independence(ragged):
    xs, ys = ragged[(4, 5)]
    base = M.voxel_counts(_dev(xs), _dev(ys), 0.1)
    assert torch.equal(base, M.voxel_counts(_dev(xs), _dev(ys), 0.1))                   # two identical calls
    rng = np.random.default_rng(1)
    xs_p = [x[rng.permutation(len(x))] for x in xs]
    ys_p = [y[rng.permutation(len(y))] for y in ys]
    assert torch.equal(base, M.voxel_counts(_dev(xs_p), _dev(ys_p), 0.1))               # points permuted
    order = rng.permutation(len(xs)).tolist()
    got = M.voxel_counts(_dev([xs[i] for i in order]), _dev([ys[i] for i in order]), 0.1)
    assert torch.equal(base[torch.as_tensor(order).cuda()], got)                        # pairs permuted
    for i in (0, 4, 6):                                                                 # a pair alone
        assert torch.equal(base[i:i + 1], M.voxel_counts(_dev(xs[i:i + 1]), _dev(ys[i:i + 1]), 0.1))


def test_more_than_one_chunk_of_tables():
    """Three pairs of 2^21 + 1 points per side: each table takes 2^24 slots, the workspace holds two, so pair 2 runs in a
    second chunk.  Integer coordinates in small boxes, every cell hit (2 M draws into at most 512 cells): the counts are the
    boxes' volumes, no host pass over 12 M points."""
    n = (1 << 21) + 1
    g = torch.Generator(device="cuda").manual_seed(3)
    xs, ys, want = [], [], []
    for k in range(3):
        x = torch.randint(0, 8, (n, 3), generator=g, device="cuda").float()
        y = torch.randint(0, 8, (n, 3), generator=g, device="cuda").float()
        y[:, 2] = torch.remainder(y[:, 2], 2 + k) + 6.0                                  # z in [6, 8 + k)
        x[:, 0] += 16.0 * k
        y[:, 0] += 16.0 * k
        xs.append(x)
        ys.append(y)
        want.append([512, 64 * (2 + k), 64 * min(2, 2 + k)])
    assert M.voxel_counts(xs, ys, 1.0).tolist() == want
    assert M.voxel_counts(xs[2:], ys[2:], 1.0).tolist() == want[2:]


def test_single_pair_above_the_workspace_is_an_error():
    big = torch.zeros(((1 << 24), 3), device="cuda")
    one = torch.zeros((1, 3), device="cuda")
    with pytest.raises(RuntimeError, match="pair 1 holds 16777217 points"):
        M.voxel_counts([one, big], [one, one], 0.1)
    assert M.voxel_counts([one], [one], 0.1).tolist() == [[1, 1, 1]]


def test_out_of_range_raises_and_the_next_call_works(ragged):
    xs, ys = ragged[(3, 3)]
    want = M.voxel_counts_host(xs, ys, 0.5)
    for bad_value in (np.nan, np.inf, np.float32(2.0 ** 20) * np.float32(0.5)):
        for side in (0, 1):
            bad = [c.copy() for c in (xs, ys)[side]]
            bad[4][1234, 1] = bad_value
            with pytest.raises(ValueError, match="out of range"):
                M.voxel_counts(_dev(bad if side == 0 else xs), _dev(bad if side == 1 else ys), 0.5)
            with pytest.raises(ValueError, match="out of range"):
                M.voxel_counts_host(bad if side == 0 else xs, bad if side == 1 else ys, 0.5)
    assert M.voxel_counts(_dev(xs), _dev(ys), 0.5).cpu().numpy().tolist() == want.tolist()
    # the lowest index, -2^20, is in range
    low = np.zeros((1, 3), np.float32)
    low[0, 2] = -np.float32(2.0 ** 20) * np.float32(0.5)
    assert _equal_host([low], [low], 0.5).tolist() == [[1, 1, 1]]


def test_cli_chamfer_voxel(tmp_path, capsys):
    rng = np.random.default_rng(4)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    xs, ys = [], []
    for i, (n, m) in enumerate([(900, 700), (1500, 1500), (64, 2000)]):
        x = (rng.standard_normal((n, 4)) * 4.0).astype(np.float32)
        y = (rng.standard_normal((m, 4)) * 4.0).astype(np.float32)
        y[:min(n, m) // 2, :3] = x[:min(n, m) // 2, :3]
        x.tofile(a_dir / f"{i:03d}.bin")
        y.tofile(b_dir / f"{i:03d}.bin")
        xs.append(x)
        ys.append(y)
    res = E.main(["chamfer", str(a_dir), str(b_dir), "--voxel", "0.5"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == res and sorted(res) == ["cd", "occupancy", "pairs", "task", "voxel"]
    h = M.voxel_scores_host(xs, ys, 0.5)
    assert res["voxel"] == 0.5 and res["pairs"] == 3
    occ = res["occupancy"]
    assert sorted(occ) == sorted(M.VOXEL_SCORES + ("voxels_result", "voxels_target", "voxels_both"))
    assert [occ["voxels_result"], occ["voxels_target"], occ["voxels_both"]] == h["counts"].sum(0).tolist()
    assert 0 < occ["voxels_both"] < min(occ["voxels_result"], occ["voxels_target"])
    for k in M.VOXEL_SCORES:
        # the mean of three fp64 ratios in [0, 1]: two additions in whatever order, each off by at most 2^-53 of a partial sum
        # <= 3, so two orders differ by at most 12 * 2^-53 in the sum and 2^-51 in the mean
        assert 0.0 < occ[k] < 1.0 and abs(occ[k] - math.fsum(h[k].tolist()) / 3) <= 2.0 ** -51
    # sharded over two ranks (no process group here: each call returns its own rank's sums): the integer totals add up
    a = E.build_parser().parse_args(["chamfer", str(a_dir), str(b_dir), "--voxel", "0.5"])
    parts = [E.cmd_chamfer(a, rank, 2, torch.device("cuda"))["occupancy"] for rank in (0, 1)]
    for key in ("voxels_result", "voxels_target", "voxels_both"):
        assert parts[0][key] + parts[1][key] == occ[key]
    plain = E.main(["chamfer", str(a_dir), str(b_dir)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(printed) == ["cd", "pairs", "task"] and printed == plain
    assert plain["cd"] == res["cd"]
