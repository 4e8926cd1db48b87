"""Farthest point sampling, host side: `fps_host`, the sequential numpy restatement of rangeldm_amd/csrc/fps.hip (the
reference tests/test_fps_gpu.py compares the kernel with, index for index), checked here by a certificate that does not use it,
and by answers worked by hand; and the host-side parts of the feature: the unchanged default of metrics.subsample, the
refusals raised before the device, the `generation --sampling` argument.

The rule.  All fp32, one rounding per operation (numpy does not contract):

    mind = +inf everywhere; sel = start
    k times:  emit sel;  d = ((dx*dx + dy*dy) + dz*dz), dx = x[i] - x[sel];  mind = min(mind, d);  mind[sel] = -inf;
              sel = the LOWEST index attaining max(mind)

The certificate.  With D the full fp32 matrix of the same expression, idx[t] (t >= 1) must be the lowest index attaining
max over the unselected i of min_{s < t} D[idx[s]][i], and the indices must be distinct.  It is evaluated from D with
boolean masks: no running array, no sentinel, no argmax.  It only ever reads the rows D[idx[s]], so it has a second form
(check_certificate_rows) that computes those k rows alone, by the same expression: k x P work, for clouds of scan size.
"""
import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M

F = np.float32


# ---- the restatement ------------------------------------------------------------------------------------------------------
def fps_host(x, k, start=0):
    """The rounds of fps.hip, one after the other: int64 [k], indices into x in selection order."""
    x = np.ascontiguousarray(np.asarray(x)[:, :3], F)
    p = len(x)
    assert 1 <= k <= p and 0 <= start < p
    mind = np.full(p, np.inf, F)
    idx = np.empty(k, np.int64)
    sel = int(start)
    with np.errstate(over="ignore"):
        for t in range(k):
            idx[t] = sel
            dx, dy, dz = x[:, 0] - x[sel, 0], x[:, 1] - x[sel, 1], x[:, 2] - x[sel, 2]
            mind = np.minimum(mind, (dx * dx + dy * dy) + dz * dz)
            mind[sel] = -np.inf
            sel = int(np.argmax(mind))                   # the first maximum: the lowest index
    return idx


def pairwise_sq(x):
    """D[a][b] = ((dx*dx + dy*dy) + dz*dz), dx = x[b] - x[a], fp32."""
    x = np.ascontiguousarray(np.asarray(x)[:, :3], F)
    dx = x[None, :, 0] - x[:, None, 0]
    dy = x[None, :, 1] - x[:, None, 1]
    dz = x[None, :, 2] - x[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def selected_rows(x, idx):
    """The rows D[idx[t]] of pairwise_sq(x) alone, fp32 [len(idx)][P], by the same expression: k x P work, not P x P."""
    x = np.ascontiguousarray(np.asarray(x)[:, :3], F)
    s = x[np.asarray(idx, np.int64)]
    dx = x[None, :, 0] - s[:, None, 0]
    dy = x[None, :, 1] - s[:, None, 1]
    dz = x[None, :, 2] - s[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def _check_rounds(name, p, idx, start, rows):
    """The assertions of the module docstring; rows(idx) gives D[idx] and is only asked once idx is known to be in range."""
    idx = [int(v) for v in idx]
    assert idx[0] == start, f"{name}: starts at {idx[0]}, not {start}"
    assert all(0 <= v < p for v in idx), f"{name}: index out of range"
    assert len(set(idx)) == len(idx), f"{name}: an index is selected twice"
    r = rows(idx)
    for t in range(1, len(idx)):
        free = np.ones(p, bool)
        free[idx[:t]] = False
        nearest = r[:t].min(0)                           # min over the selected s of D[s][i]
        top = nearest[free].max()
        want = int(np.flatnonzero(free & (nearest == top))[0])
        assert idx[t] == want, f"{name}: round {t} selected {idx[t]}, the lowest farthest index is {want}"


def check_certificate(name, x, idx, start, d=None):
    """The certificate on any index list claimed for the cloud x, from the full matrix D (computed here unless given)."""
    d = pairwise_sq(x) if d is None else d
    _check_rounds(name, len(x), idx, start, lambda sel: d[sel])


def check_certificate_rows(name, x, idx, start):
    """The same certificate from the len(idx) rows of D it reads, computed on their own: for clouds whose D does not fit."""
    _check_rounds(name, len(x), idx, start, lambda sel: selected_rows(x, sel))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def lidar_like(rng, n):
    """A spinning-sensor sweep: ranges 3 .. 70 m (ground-heavy), 64 beams between -25 and +3 degrees, any azimuth."""
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.choice(np.linspace(-25.0, 3.0, 64), n))
    r = np.minimum(3.0 + rng.exponential(12.0, n), 70.0)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F)


def lattice(rng, n):
    """Integer coordinates in [-3, 3]^3: every distance is exact, ties and duplicate points are everywhere."""
    return rng.integers(-3, 4, (n, 3)).astype(F)


def half_duplicates(rng, n):
    """Half the points are copies of the others, in a shuffled order."""
    base = lidar_like(rng, n - n // 2)
    both = np.concatenate([base, base[rng.integers(0, len(base), n // 2)]])
    return both[rng.permutation(n)]


CLOUD_KINDS = {"lidar": lidar_like, "lattice": lattice, "half_duplicates": half_duplicates}


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(CLOUD_KINDS))
def test_fps_host_passes_the_certificate(kind):
    rng = np.random.default_rng(20250131)
    for p, k, start in ((1, 1, 0), (2, 2, 1), (65, 65, 64), (300, 300, 17), (1500, 40, 0)):
        x = CLOUD_KINDS[kind](rng, p)
        idx = fps_host(x, k, start)
        assert idx.dtype == np.int64 and idx.shape == (k,)
        check_certificate(f"{kind} P={p} k={k}", x, idx, start)
        if k == p:
            assert sorted(idx.tolist()) == list(range(p))


def test_the_certificate_refuses_wrong_answers():
    x = lidar_like(np.random.default_rng(3), 50)
    good = fps_host(x, 10, 4)
    same = np.ones((6, 3), F)
    assert np.array_equal(selected_rows(x, good).view(np.int32), pairwise_sq(x)[good].view(np.int32))      # the same rows, bit for bit
    for check in (check_certificate, check_certificate_rows):
        check("good", x, good, 4)
        for bad in (good[[0, 2, 1] + list(range(3, 10))], np.concatenate([good[:9], good[:1]])):
            with pytest.raises(AssertionError):
                check("bad", x, bad, 4)
        # the tie rule is part of it: on a cloud of identical points any order is "farthest", only one is the lowest index
        with pytest.raises(AssertionError):
            check("tie", same, [2, 1, 0], 2)
        check("tie", same, [2, 0, 1], 2)
    # what the full form cannot see for lack of memory, the row form refuses as well: a wrong start, an index outside the
    # cloud (before any row is formed from it), a later round's lower-index tie
    for bad, start in ((good, 5), ([4, 50], 4), ([4, -1], 4)):
        with pytest.raises(AssertionError):
            check_certificate_rows("bad", x, bad, start)
    far = np.zeros((40, 3), F)
    far[[7, 31], 0] = 3.0                                # two points equally far from the rest: 7 is the answer, 31 is not
    check_certificate_rows("tie", far, [0, 7], 0)
    with pytest.raises(AssertionError):
        check_certificate_rows("tie", far, [0, 31], 0)


def test_known_answers():
    # points on a line, x = 0 1 2 3 10 from index 0: 10 is farthest; then 3 (d^2 = 9 from 0); then 1 and 2 tie at 1 -> 1
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], F)
    assert fps_host(line, 5, 0).tolist() == [0, 4, 3, 1, 2]
    assert fps_host(line, 3, 2).tolist() == [2, 4, 0]
    # the 3 x 3 x 3 lattice, point (a, b, c) at index 9 a + 3 b + c, from the corner (0, 0, 0): the opposite corner (d^2 = 12);
    # then the six permutations of (0, 1, 2) are 5 from both (every other point is closer to one of them) -> the lowest,
    # (0, 1, 2) = index 5.  The arithmetic is exact, so the whole order is decided by the lowest-index rule: certified.
    grid = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F)
    assert grid[5].tolist() == [0, 1, 2] and grid[26].tolist() == [2, 2, 2]
    idx = fps_host(grid, 27, 0)
    assert idx[:3].tolist() == [0, 26, 5] and sorted(idx.tolist()) == list(range(27))
    check_certificate("lattice", grid, idx, 0)
    # identical points: every distance is 0, the sentinel alone orders them -- the start, then 0 .. k-1 without it
    same = np.full((9, 3), 2.5, F)
    assert fps_host(same, 5, 3).tolist() == [3, 0, 1, 2, 4]
    assert fps_host(same, 9, 0).tolist() == list(range(9))
    # extra columns are not coordinates
    wide = np.concatenate([line, np.arange(5, dtype=F)[::-1, None] * 100], 1)
    assert fps_host(wide, 5, 0).tolist() == [0, 4, 3, 1, 2]


def test_the_default_sub_sample_is_unchanged():
    cloud = torch.arange(5000 * 4, dtype=torch.float32).view(5000, 4)
    for n, seed in ((2048, 7), (100, 0), (4999, 123456)):
        want = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(5000, size=n, replace=False))
        assert torch.equal(M.subsample(cloud, n, seed), cloud[torch.from_numpy(want)])
        assert torch.equal(M.subsample(cloud, n, seed, method="random"), cloud[torch.from_numpy(want)])
        assert torch.equal(M.subsample_batch([cloud, cloud[:n]], n, [seed, seed + 1])[0], cloud[torch.from_numpy(want)])
    # a cloud that is short enough is returned whole, whatever the method (no device involved)
    short = cloud[:100]
    for method in ("random", "fps"):
        assert torch.equal(M.subsample(short, 100, 3, method=method), short)
        assert torch.equal(M.subsample(short, 2048, 3, method=method), short)
        assert all(torch.equal(c, short) for c in M.subsample_batch([short, short], 100, [1, 2], method))


def test_constants_mirror_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rangeldm_hip.h")).read()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert M.FPS_BLOCK == value("RLDM_FPS_BLOCK")
    assert M.FPS_RESIDENT_POINTS == value("RLDM_FPS_RESIDENT_POINTS")
    assert M.FPS_MAX_POINTS == value("RLDM_FPS_MAX_POINTS") >= 262144
    assert M.FPS_RESIDENT_POINTS % M.FPS_BLOCK == 0 and M.FPS_RESIDENT_POINTS >= 65536
    assert M.FPS_STAGED_POINTS == value("RLDM_FPS_STAGED_POINTS")
    assert M.FPS_GROUP_POINTS == value("RLDM_FPS_GROUP_POINTS")
    # whole groups of whole slots are staged, and the resident tier is whole groups: the sizes the GPU tests derive hold
    assert M.FPS_GROUP_POINTS % M.FPS_BLOCK == 0 and M.FPS_STAGED_POINTS % M.FPS_GROUP_POINTS == 0
    assert M.FPS_STAGED_POINTS < M.FPS_RESIDENT_POINTS and M.FPS_RESIDENT_POINTS % M.FPS_GROUP_POINTS == 0


def test_refusals_come_before_the_device():
    a, b = torch.zeros((5, 3)), torch.zeros((9, 4))
    with pytest.raises(ValueError, match="bogus"):
        M.subsample(b, 4, 0, method="bogus")
    with pytest.raises(ValueError, match="bogus"):
        M.subsample_batch([b], 4, [0], "bogus")
    with pytest.raises(ValueError, match=r"cloud 1 holds 5 points, fewer than k = 6"):
        M.farthest_point_sample([b, a], 6)
    with pytest.raises(ValueError, match="k must be"):
        M.farthest_point_sample([a], 0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        c = torch.zeros((7, 3))
        c[4, 1] = bad
        with pytest.raises(ValueError, match="cloud 2 holds non-finite"):
            M.farthest_point_sample([a, a, c], 3)
        with pytest.raises(ValueError, match="non-finite"):
            M.subsample(c, 3, 0, method="fps")
    with pytest.raises(ValueError, match="start"):
        M.farthest_point_sample([a], 2, start=5)
    with pytest.raises(ValueError, match="start"):
        M.farthest_point_sample([a, a], 2, start=[0])
    with pytest.raises(ValueError, match="empty"):
        M.farthest_point_sample([a, torch.zeros((0, 3))], 1)
    with pytest.raises(ValueError):
        M.farthest_point_sample(torch.zeros((2, 5, 2)), 1)                 # xyz needed
    with pytest.raises(ValueError):
        M.farthest_point_sample(torch.zeros((2, 5, 3)), 6)                 # padded form: k above every cloud


def test_generation_sampling_argument():
    from rangeldm_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["generation", "g", "r"]).sampling == "random"
    assert ap.parse_args(["generation", "g", "r", "--sampling", "fps", "--emd"]).sampling == "fps"
    with pytest.raises(SystemExit):
        ap.parse_args(["generation", "g", "r", "--sampling", "bogus"])
    with pytest.raises(SystemExit):
        ap.parse_args(["chamfer", "a", "b", "--sampling", "fps"])
