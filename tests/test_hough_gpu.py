"""Sensor tables by Hough voting on the device (rangeldm_amd/csrc/hough.hip; rangeldm_amd/sensor.py; `calibrate_sensor`).

Votes, row maxima and beam ids are integers: every case asks for EQUALITY with the numpy statements of sensor.py.  The
per-beam moments are fp64 sums in another (fixed) order than numpy's: counts exact, sums within 1e-12 of the sum of the
absolute terms, and the same bits from two calls.  estimate_sensor must pass the gates of test_hough_host.py against the
truth, give the host pipeline's Hough-stage tables exactly and its refined tables to 1e-10, and its tables must project a
cloud onto the same pixels as the shipped KITTI-360 class.
"""
import json

import numpy as np
import pytest
import torch

import hough_util as U
from rangeldm_amd import calibrate_sensor
from rangeldm_amd import sensor as S
from rangeldm_amd.range_image import point_cloud_to_range_image_KITTI, point_cloud_to_range_image_tables

pytestmark = pytest.mark.gpu

SMALL = S.HoughGrid(-0.06, 0.04, 13, 0.0, 0.01, 37)              # 13 rows: ragged last row block; 37 bins: odd row pitch
# row 0 is theta = 0 exactly (tan 0: h = z), h bins of 1/4 m from 0 to 2: the limits can be hit exactly
EXACT = S.HoughGrid(-0.005, 0.01, 3, 0.0, 0.25, 8)


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _votes(clouds, grid, **kw):
    acc = S.HoughAccumulator(grid).add(_dev(clouds), **kw)
    v = acc.votes()
    assert v.dtype == torch.uint32 and v.is_cuda and tuple(v.shape) == (grid.n_theta, grid.n_h)
    return acc, v.cpu().numpy()


def _equal_host(clouds, grid):
    acc, got = _votes(clouds, grid)
    want = S.hough_votes_host(clouds, grid)
    assert np.array_equal(got, want)
    assert acc.points == int((S.pack_host(clouds, grid.d_min, grid.d_max)[:, 0] >= 0).sum())
    mx, arg = acc.row_peaks()
    hm, ha = S.row_peaks_host(want)
    assert mx.dtype == torch.int64 and mx.cpu().numpy().tolist() == hm.tolist() and arg.cpu().numpy().tolist() == ha.tolist()
    return want


def _cloud(n, seed, stride=3):
    """n returns of an 8-beam sensor whose lines cross the SMALL grid, in random order, `stride` columns."""
    rng = np.random.default_rng(seed)
    incl, height = np.linspace(-0.04, 0.44, 8), np.linspace(0.33, 0.02, 8)
    k = rng.integers(0, 8, n)
    r = np.exp(rng.uniform(np.log(2.5), np.log(80.0), n))
    a = rng.uniform(-np.pi, np.pi, n)
    pts = rng.standard_normal((n, stride))
    pts[:, 0], pts[:, 1] = r * np.cos(incl[k]) * np.cos(a), r * np.cos(incl[k]) * np.sin(a)
    pts[:, 2] = height[k] - r * np.sin(incl[k])
    return pts.astype(np.float32)


@pytest.fixture(scope="module")
def kitti():
    """The KITTI-360 recovery fixture and the host pipeline over it, computed once."""
    sweeps = U.kitti_sweeps()
    votes = S.hough_votes_host(sweeps, U.GRID)
    peaks = S.row_peaks_host(votes)
    hough = S.tables_from_peaks(peaks, None, sweeps, 64, U.GRID, U.MIN_SEPARATION, False, None)
    fine = S.tables_from_peaks(peaks, S.refine_beams_host, sweeps, 64, U.GRID, U.MIN_SEPARATION, True, None)
    return dict(sweeps=sweeps, votes=votes, hough=hough, fine=fine)


# ---- vote ------------------------------------------------------------------------------------------------------------
def test_vote_one_point():
    want = _equal_host([np.array([[3.0, 4.0, 0.1]], np.float32)], SMALL)
    assert 1 <= int(want.sum()) <= SMALL.n_theta and want.max() == 1


def test_vote_257_points_on_a_1x1_grid():
    g = S.HoughGrid(0.0, 0.1, 1, -1000.0, 2000.0, 1)
    want = _equal_host([_cloud(257, 1)], g)
    assert want.tolist() == [[257]]


def test_vote_slices_remainder_and_ragged_row_block():
    n = 2 * 1024 + 301
    rows, slice_len = S.vote_shape(n, SMALL)
    assert rows < SMALL.n_theta and SMALL.n_theta % rows != 0, "the last row block must be ragged"
    assert n > 2 * slice_len and n % slice_len != 0, "two full point slices and a remainder"
    want = _equal_host([_cloud(n, 2, stride=4)], SMALL)
    assert want.sum() > n // 4 and (want.sum(1) > 0).all()    # every row of both row blocks holds votes


def test_vote_4096_bins():
    g = S.HoughGrid(-0.06, 0.1, 5, -0.5, 2.5e-4, 4096)
    rows, _ = S.vote_shape(3000, g)
    assert rows * g.n_h * 4 <= 32768 and g.n_theta % rows != 0
    want = _equal_host([_cloud(3000, 3)], g)
    assert want[:, 2048:].sum() > 0 and want[:, :2048].sum() > 0


def test_vote_70000_identical_points():
    """Every lane of every wave on one counter, and a count above 16 bits."""
    want = _equal_host([np.tile(np.array([[3.0, 4.0, 0.1]], np.float32), (70000, 1))], SMALL)
    assert want.max() == 70000 and set(np.unique(want).tolist()) == {0, 70000}


def test_vote_edges():
    f = np.float32
    up, down = (lambda v, t=np.inf: np.nextafter(f(v), f(t))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    pts = np.array([
        [np.nan, 3.0, 0.5], [3.0, np.nan, 0.5], [3.0, 4.0, np.nan], [np.inf, 0.0, 0.5], [0.0, -np.inf, 0.5], [3.0, 4.0, np.inf],
        [3.0, 4.0, -np.inf], [1e30, 0.0, 0.5],                                         # d overflows to inf
        [2.0, 0.0, 0.5], [down(2.0), 0.0, 0.5], [up(2.0), 0.0, 0.5],                   # d = d_min, below, above
        [0.0, 90.0, 0.5], [0.0, down(90.0), 0.5], [0.0, up(90.0), 0.5],                # d = d_max, below, above
        [3.0, 4.0, 0.0], [3.0, 4.0, -1e-45], [3.0, 4.0, down(0.0)], [3.0, 4.0, -0.3],  # h = h_min, a denormal below it, below
        [3.0, 4.0, 2.0], [3.0, 4.0, down(2.0)], [3.0, 4.0, up(2.0)],                   # h = h_min + n_h * h_step: out; below it: in
        [3.0, 4.0, 1e30], [3.0, 4.0, -1e30], [3.0, 4.0, 3e38],
        [3.0, 4.0, 0.25], [3.0, 4.0, down(0.25)],                                      # a bin boundary
    ], np.float32)
    packed = S.pack(torch.from_numpy(pts).cuda(), EXACT.d_min, EXACT.d_max).cpu().numpy()
    want_packed = S.pack_host([pts], EXACT.d_min, EXACT.d_max)
    assert np.array_equal(packed.view(np.uint32), want_packed.view(np.uint32))
    assert (packed[:8, 0] == -1).all() and packed[8:14, 0].tolist() == [2.0, -1.0, float(up(2.0)), 90.0, float(down(90.0)), -1.0]
    want = _equal_host([pts], EXACT)
    # row 0 (tan 0, h = z): z = 0.5 four times (bin 2), z = 0 and 0.25- (bin 0), 2- (bin 7), 0.25 (bin 1); nothing else
    assert want[0].tolist() == [2, 1, 4, 0, 0, 0, 0, 1]


def test_vote_two_adds_equal_one():
    a, b = _cloud(1500, 4), _cloud(900, 5, stride=5)
    acc = S.HoughAccumulator(SMALL).add(_dev([a])).add(_dev([b]))
    both, want = _votes([np.concatenate([a, b[:, :3]], 0)], SMALL)
    assert np.array_equal(acc.votes().cpu().numpy(), want) and acc.points == both.points
    assert np.array_equal(want, S.hough_votes_host([a, b], SMALL))


def test_vote_empty_cloud_within_a_batch_and_padded_batch():
    a, b = _cloud(700, 6), _cloud(300, 7)
    want = _equal_host([a, np.zeros((0, 3), np.float32), b], SMALL)
    pad = torch.full((3, 700, 3), 5.0).cuda()
    pad[0] = torch.from_numpy(a).cuda()
    pad[2, :300] = torch.from_numpy(b).cuda()
    acc = S.HoughAccumulator(SMALL).add(pad, lengths=torch.tensor([700, 0, 300]))
    assert np.array_equal(acc.votes().cpu().numpy(), want)
    assert S.HoughAccumulator(SMALL).add([np.zeros((0, 4), np.float32)]).points == 0


def test_vote_kitti_fixture(kitti):
    _, got = _votes(kitti["sweeps"], U.GRID)
    assert np.array_equal(got, kitti["votes"])


# ---- row_max ---------------------------------------------------------------------------------------------------------
def test_row_max_ties_zero_rows_and_counts_above_2_31():
    g = S.HoughGrid(-0.06, 0.01, 6, 0.0, 0.01, 600)
    v = np.zeros((6, 600), np.uint32)
    v[1, [300, 5]] = 9                     # a tie held by two threads: the lower bin
    v[2, [10, 266]] = 4                    # a tie inside one thread's stride
    v[2, 599] = 3
    v[3, 599] = 1                          # the last bin
    v[4, [7, 100, 400]] = [5, 3_000_000_000, 3_000_000_000]        # compared as unsigned
    v[5, :] = 2                            # a whole row tied
    acc = S.HoughAccumulator(g)
    acc.votes().copy_(torch.from_numpy(v))
    mx, arg = acc.row_peaks()
    assert mx.cpu().tolist() == [0, 9, 4, 1, 3_000_000_000, 2] and arg.cpu().tolist() == [0, 5, 10, 599, 100, 0]
    hm, ha = S.row_peaks_host(v)
    assert hm.tolist() == mx.cpu().tolist() and ha.tolist() == arg.cpu().tolist()


# ---- assign ----------------------------------------------------------------------------------------------------------
def _assign_equal(packed, cand, tol):
    got = S.assign(torch.from_numpy(packed).cuda(), cand, tol)
    assert got.dtype == torch.int16 and got.is_cuda
    want = S.assign_host(packed, cand, tol)
    assert np.array_equal(got.cpu().numpy(), want)
    return want


def test_assign_by_hand():
    cand = np.array([[0.0, 1.0], [0.0, 1.0], [0.5, 0.0]], np.float32)
    # on the two identical beams (the lower id); on beam 2; a residual equal to tol (out); invalid
    packed = np.array([[4.0, 1.0], [2.0, -1.0], [4.0, -3.0], [-1.0, 0.0]], np.float32)
    assert _assign_equal(packed, cand, 0.25).tolist() == [0, 2, -1, -1]
    assert _assign_equal(packed, cand, float(np.nextafter(np.float32(0.25), np.float32(1)))).tolist() == [0, 2, 2, -1]


@pytest.mark.parametrize("beams", [1, 64, 256])
def test_assign_equals_host(kitti, beams):
    packed = S.pack_host(kitti["sweeps"][:1], 2.0, 90.0)[:20001]
    packed[::97, 0] = -1.0                                   # invalid points in between
    rng = np.random.default_rng(beams)
    if beams == 256:                                         # candidates closer together than tol: many near-ties
        incl, height = np.sort(rng.uniform(-0.04, 0.44, beams)), rng.uniform(0.1, 0.22, beams)
    else:                                                    # the sensor's own beams, slightly off (beams = 1: beam 10 alone)
        incl, height = (U.KITTI_INCL + 2e-4)[10:10 + beams], (U.KITTI_HEIGHT - 1e-3)[10:10 + beams]
    want = _assign_equal(packed, S.candidates(incl, height), 1e-3)
    assert (want[::97] == -1).all() and len(np.unique(want[want >= 0])) > beams // 2


# ---- moments ---------------------------------------------------------------------------------------------------------
def test_moments(kitti):
    packed = S.pack_host(kitti["sweeps"], 2.0, 90.0)
    cand = S.candidates(kitti["hough"].incl, kitti["hough"].height)[:-1]       # 63 beams: the last group of four is ragged
    ids = S.assign_host(packed, cand, 1e-3)
    ids[ids == 7] = -1                                                       # a beam without points
    counts, sums, mags = S.moments_host(packed, ids, len(cand), return_abs=True)
    dp, di = torch.from_numpy(packed).cuda(), torch.from_numpy(ids).cuda()
    c1, s1 = S.moments(dp, di, len(cand))
    c2, s2 = S.moments(dp, di, len(cand))
    assert c1.dtype == torch.int64 and s1.dtype == torch.float64 and tuple(s1.shape) == (63, 4)
    assert c1.cpu().numpy().tolist() == counts.tolist() and counts[7] == 0 and counts.sum() > 90000
    assert s1[7].cpu().tolist() == [0.0] * 4
    err = np.abs(s1.cpu().numpy() - sums)
    print("moments: worst |device - host| / sum |terms| = %.3g" % float((err / np.maximum(mags, 1e-300)).max()))
    assert (err <= 1e-12 * mags).all()
    assert np.array_equal(s1.cpu().numpy().view(np.uint64), s2.cpu().numpy().view(np.uint64)) and torch.equal(c1, c2)
    c0, s0 = S.moments(dp[:0], di[:0], 3)
    assert c0.cpu().tolist() == [0, 0, 0] and s0.abs().sum().item() == 0.0


# ---- estimate_sensor -------------------------------------------------------------------------------------------------
def _estimate_checks(sweeps, beams, incl, height, refined_gate, host_hough, host_fine):
    hough = S.estimate_sensor(sweeps, beams, U.GRID, U.MIN_SEPARATION, refine=False)
    e = U.worst(hough, incl, height)
    print("hough stage: %.3f rows, %.3f bins" % (e[0] / U.GRID.theta_step, e[1] / U.GRID.h_step))
    assert e[0] <= U.HOUGH_GATE[0] and e[1] <= U.HOUGH_GATE[1]
    assert hough.incl.tolist() == host_hough.incl.tolist() and hough.height.tolist() == host_hough.height.tolist()
    assert hough.votes.tolist() == host_hough.votes.tolist()
    fine = S.estimate_sensor(sweeps, beams, U.GRID, U.MIN_SEPARATION)
    e = U.worst(fine, incl, height)
    print("refined: %.3g rad, %.3g m" % e)
    assert e[0] <= refined_gate[0] and e[1] <= refined_gate[1]
    assert fine.support.tolist() == host_fine.support.tolist()
    assert np.abs(fine.incl - host_fine.incl).max() <= 1e-10 and np.abs(fine.height - host_fine.height).max() <= 1e-10
    return fine


def test_estimate_sensor_kitti(kitti):
    _estimate_checks(_dev(kitti["sweeps"]), 64, U.KITTI_INCL, U.KITTI_HEIGHT, U.KITTI_REFINED_GATE, kitti["hough"], kitti["fine"])


def test_estimate_sensor_jittered():
    sweeps = U.jitter_sweeps()
    host_hough = S.estimate_sensor_host(sweeps, 16, U.GRID, U.MIN_SEPARATION, refine=False)
    host_fine = S.estimate_sensor_host(sweeps, 16, U.GRID, U.MIN_SEPARATION)
    _estimate_checks(sweeps, 16, U.TWO_GROUP_INCL, U.TWO_GROUP_HEIGHT, U.JITTER_REFINED_GATE, host_hough, host_fine)


def test_round_trip_through_project(kitti):
    """Tables estimated from the fixture project a cloud of the shipped sensor onto the pixels the shipped class fills."""
    tables = S.estimate_sensor(_dev(kitti["sweeps"]), 64, U.GRID, U.MIN_SEPARATION)
    shipped, mine = point_cloud_to_range_image_KITTI(), point_cloud_to_range_image_tables(tables)
    assert mine.H == 64 and mine.width == 1024
    rng = np.random.default_rng(11)
    r = np.exp(rng.uniform(np.log(2.5), np.log(80.0), (1, 1, 1024, 64)))
    img = np.concatenate([(r - 20.0) / 40.0, rng.uniform(0, 1, r.shape)], 1).astype(np.float32)
    pc = shipped.to_pc_torch(torch.from_numpy(img).cuda())[0]
    pc = pc[torch.from_numpy(rng.uniform(size=pc.shape[0]) >= 0.3).cuda()]
    a, b = shipped.project(pc), mine.project(pc)
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["car_window_mask"], b["car_window_mask"])
    share = float(a["mask"].float().mean())
    assert 0.5 < share < 1.0
    assert (a["jpg"][0] - b["jpg"][0]).abs().max().item() <= 1e-5          # the same returns, ranges from heights 1e-5 m apart


# ---- command line ----------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    folder = tmp_path / "clouds"
    folder.mkdir()
    for i in range(4):
        c = U.synth_sweep(U.KITTI_INCL, U.KITTI_HEIGHT, 256, 20 + i)
        if i % 2:
            np.save(str(folder / f"{i}.npy"), c)
        else:
            np.concatenate([c, np.full((len(c), 1), 0.5, np.float32)], 1).tofile(str(folder / f"{i}.bin"))
    out, js = tmp_path / "sensor.json", tmp_path / "result.json"
    g = U.GRID
    calibrate_sensor.main([str(folder), "--beams", "64", "--out", str(out), "--json", str(js), "--width", "256",
                           "--theta-min", str(g.theta_min), "--theta-step", str(g.theta_step), "--n-theta", str(g.n_theta),
                           "--h-min", str(g.h_min), "--h-step", str(g.h_step), "--n-h", str(g.n_h), "--min-separation", "4"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res == json.loads(js.read_text())
    assert {"height", "incl", "votes", "support", "points", "fill", "grid", "files"} <= set(res)
    assert all(len(res[k]) == 64 for k in ("height", "incl", "votes", "support")) and res["files"] == 4
    assert res["points"] >= sum(res["support"]) > 40000
    assert set(res["fill"]) == {"estimated", "spherical"}
    # uniform inclinations and zero heights put returns of neighbouring beams into one row: holes the estimated tables do not leave
    assert 0.0 < res["fill"]["spherical"] < res["fill"]["estimated"] <= 1.0
    tables = S.SensorTables.load(str(out))
    e = U.worst(tables, U.KITTI_INCL, U.KITTI_HEIGHT)
    assert e[0] <= U.KITTI_REFINED_GATE[0] and e[1] <= U.KITTI_REFINED_GATE[1] and tables.grid == g
