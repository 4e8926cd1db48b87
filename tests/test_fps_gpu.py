"""Farthest point sampling on the device (rangeldm_amd/csrc/fps.hip: fps_kernel; rangeldm_amd.metrics.farthest_point_sample /
subsample(method="fps") / subsample_batch; `evaluate generation --sampling fps`).

The kernel's indices are compared EXACTLY with tests/test_fps_host.py's sequential numpy restatement `fps_host`, at cloud
sizes around the kernel's own boundaries (one wave, the workgroup, a few slots per lane, the resident tier and the first point
past it), on LiDAR-like clouds, on integer lattices (dense ties: a reduction that breaks the lowest-index rule at lane, wave or
workgroup level fails there) and on clouds where half the points are duplicates (the sentinel).  The device output is also put
through the host test's certificate, which would hold even if the restatement were wrong.  TIER_SIZES then walks the kernel's
three coordinate / min-distance paths (LDS-staged slots, slots re-read in groups of four, the workspace past the resident
points) at every boundary between them and inside partially filled groups, with a start in each tier and with the protocol's
k = 2 048 at the size of a real scan; there the certificate is the row form, k x P.  Then the properties the drivers rely
on: prefixes, an entry depends on its cloud alone (batches, strides, starts), the sub-sampling wrappers, and the driver as one
process and as two ranks.  No test provokes the size cap or any fault on the device.
"""
import functools
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M
from test_emd_host import EPS, auction_host
from test_fps_host import CLOUD_KINDS, check_certificate, check_certificate_rows, fps_host, lidar_like, pairwise_sq
from test_generation_metrics import _run_evaluate

pytestmark = pytest.mark.gpu

B, R = M.FPS_BLOCK, M.FPS_RESIDENT_POINTS
SMALL_SIZES = (1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 3)
LARGE_SIZES = (R, R + 1)
# The tiers.  Slot j of a lane is point lane + j B.  The first S points' coordinates come from LDS, the others are re-read in
# groups of G points (four slots per lane) through a running offset clamped to the last point; past R points the min-distances
# live in the workspace, again G points at a time.  S + B + 5: a re-read group of one full slot, five lanes of a second and two
# empty slots; S + G + 1, R + G + 1: a group that holds a single point; SCAN: a 64 x 1024 range image less its invalid pixels.
G, S = M.FPS_GROUP_POINTS, M.FPS_STAGED_POINTS
SCAN = 40123
TIER_SIZES = (G - 1, G, G + 1, S - 1, S, S + 1, S + B + 5, S + G + 1, SCAN, R - 1, R + B + 5, R + G, R + G + 1, 2 * R + 3)


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _fps(clouds, k, start=0):
    out = M.farthest_point_sample(_dev(clouds), k, start=start)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(clouds), k) and out.is_cuda
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _tier_cloud(kind, p):
    """One seeded cloud per (kind, size), shared by the tests below; nobody writes to it."""
    return CLOUD_KINDS[kind](np.random.default_rng([20250720, sorted(CLOUD_KINDS).index(kind), p]), p)


def _ks(p):
    return sorted({k for k in (1, 2, 17, p) if k <= p})


@pytest.mark.parametrize("kind", sorted(CLOUD_KINDS))
def test_kernel_equals_fps_host_exactly_and_is_certified(kind):
    rng = np.random.default_rng(20250201)
    for p in SMALL_SIZES:
        x = CLOUD_KINDS[kind](rng, p)
        d = pairwise_sq(x)
        start = int(rng.integers(p))
        for k in _ks(p):
            got = _fps([x], k, start)[0]
            # the certificate first: it does not depend on the restatement
            check_certificate(f"{kind} P={p} k={k} (device)", x, got, start, d)
            want = fps_host(x, k, start)
            assert np.array_equal(got, want), (kind, p, k, int((got != want).argmax()))
            assert len(set(got.tolist())) == k
    for p in LARGE_SIZES:                                # large P is cheap when k is small
        x = CLOUD_KINDS[kind](rng, p)
        start = p - 1                                    # (the last point: in the workspace tier of the larger cloud)
        got = _fps([x], 8, start)[0]
        assert np.array_equal(got, fps_host(x, 8, start)), (kind, p)
        assert len(set(got.tolist())) == 8


@pytest.mark.parametrize("p", TIER_SIZES)
@pytest.mark.parametrize("kind", sorted(CLOUD_KINDS))
def test_every_tier_boundary_equals_fps_host_exactly_and_is_certified(kind, p):
    x = _tier_cloud(kind, p)
    for start in [p - 1, 0] + ([S] if S < p else []):    # the last point's tier, the LDS tier, the first re-read point
        got = _fps([x], 17, start)[0]
        check_certificate_rows(f"{kind} P={p} start={start} (device)", x, got, start)
        want = fps_host(x, 17, start)
        assert np.array_equal(got, want), (kind, p, start, int((got != want).argmax()))
        assert len(set(got.tolist())) == 17


@pytest.mark.parametrize("kind", sorted(CLOUD_KINDS))
def test_the_protocols_2048_points_of_a_scan(kind):
    x = _tier_cloud(kind, SCAN)
    start = SCAN - 1
    got = _fps([x], 2048, start)[0]
    check_certificate_rows(f"{kind} P={SCAN} k=2048, its first 17 (device)", x, got[:17], start)
    want = fps_host(x, 2048, start)
    assert np.array_equal(got, want), (kind, int((got != want).argmax()))
    assert len(set(got.tolist())) == 2048


def test_identical_points_past_the_resident_tier_are_each_selected_once():
    # every distance is 0, so the sentinel alone orders the rounds: the start, then 0, 1, 2, ... without it (fps_host gives
    # that on 9 points in test_fps_host.py's known answers; P sequential numpy rounds over P points would take about a minute).
    # With k = P each of the five workspace points, the start among them, has to lose to every resident index and still be
    # emitted exactly once -- the only shape at which a workspace sentinel that is not kept shows.
    p, start = R + 5, R + 2
    got = _fps([np.full((p, 3), 2.5, np.float32)], p, start)[0]
    assert np.array_equal(got, np.array([start] + [i for i in range(p) if i != start]))


def test_prefix_property():
    rng = np.random.default_rng(7)
    clouds = [lidar_like(rng, 3000), CLOUD_KINDS["lattice"](rng, 1500), CLOUD_KINDS["half_duplicates"](rng, 70)]
    long, short = _fps(clouds, 64), _fps(clouds, 16)
    assert np.array_equal(long[:, :16], short)


def test_a_ragged_batch_equals_the_one_by_one_calls():
    rng = np.random.default_rng(8)
    tiers = [S + B + 5, SCAN, R + G + 1]                 # all three tiers in one launch, workspace offsets of no round size
    sizes = [p for p in SMALL_SIZES if p >= 17] + list(LARGE_SIZES) + tiers
    kinds = sorted(CLOUD_KINDS)
    clouds = [CLOUD_KINDS[kinds[i % 3]](rng, p) for i, p in enumerate(sizes)]
    starts = [int(rng.integers(len(c))) for c in clouds]
    batch = _fps(clouds, 17, starts)
    assert batch[:, 0].tolist() == starts                # a per-cloud start is honoured
    for i, (c, s) in enumerate(zip(clouds, starts)):
        assert np.array_equal(batch[i], _fps([c], 17, s)[0]), sizes[i]
    for i in [0] + [sizes.index(p) for p in tiers]:
        assert np.array_equal(batch[i], fps_host(clouds[i], 17, starts[i])), sizes[i]
    # the padded form with lengths is the same batch
    small = [c for c in clouds if len(c) <= 2 * B + 3]
    padded = torch.zeros((len(small), 2 * B + 3, 3))
    for i, c in enumerate(small):
        padded[i, :len(c)] = torch.from_numpy(c)
    got = M.farthest_point_sample(padded.cuda(), 17, x_lengths=[len(c) for c in small], start=starts[:len(small)])
    assert np.array_equal(got.cpu().numpy(), batch[:len(small)])


def test_strides_3_4_5():
    rng = np.random.default_rng(9)
    # (the third cloud reaches the re-read slots, whose byte offsets depend on the stride; the staged slots' do not)
    clouds = [lidar_like(rng, 2 * B + 3), CLOUD_KINDS["lattice"](rng, 700), _tier_cloud("half_duplicates", S + B + 5)]
    starts = [5, 699, S + B + 4]
    want = _fps(clouds, 33, starts)
    assert np.array_equal(want[2], fps_host(clouds[2], 33, starts[2]))
    for k in (4, 5):
        wide = [np.concatenate([c, rng.uniform(-1e3, 1e3, (len(c), k - 3)).astype(np.float32)], 1) for c in clouds]
        assert np.array_equal(_fps(wide, 33, starts), want), k


def test_subsample_fps_and_the_batched_form():
    rng = np.random.default_rng(10)
    clouds = [np.concatenate([lidar_like(rng, p), rng.uniform(0, 1, (p, 1)).astype(np.float32)], 1) for p in (900, 64, 2500, 50)]
    dev = _dev(clouds)
    seeds = [11, 12, 13, 14]
    batch = M.subsample_batch(dev, 64, seeds, "fps")
    for c, d, s, got in zip(clouds, dev, seeds, batch):
        one = M.subsample(d, 64, s, method="fps")
        assert torch.equal(one, got)
        if len(c) <= 64:
            assert torch.equal(got, d)                   # all points, as they are
            continue
        start = int(np.random.Generator(np.random.PCG64(s)).integers(len(c)))
        idx = np.sort(fps_host(c, 64, start))            # the FPS set in the cloud's original order
        assert got.shape == (64, 4) and np.array_equal(got.cpu().numpy(), c[idx])
    assert not torch.equal(M.subsample(dev[0], 64, 99, method="fps"), batch[0])          # the seed (the start) matters


def test_scans_cut_by_fps_then_matched_by_emd():
    # the two restatement-defined kernels as the generation metrics chain them, at the sizes scans have: one call of each
    rng = np.random.default_rng(12)
    sizes = [int(p) + (int(p) % B == 0) for p in rng.integers(13000, 45001, 6)]
    assert all(13000 <= p <= 45000 and p % B for p in sizes) and max(sizes) > S
    clouds = [lidar_like(rng, p) for p in sizes]
    seeds = [21, 22, 23, 24, 25, 26]
    cut = M.subsample_batch(_dev(clouds), 256, seeds, method="fps")
    want = []
    for c, s, got in zip(clouds, seeds, cut):
        start = int(np.random.Generator(np.random.PCG64(s)).integers(len(c)))
        want.append(c[np.sort(fps_host(c, 256, start))])
        assert np.array_equal(got.cpu().numpy(), want[-1]), len(c)
    emd = M.emd_pairs(cut[:3], cut[3:], eps=EPS).cpu().numpy()
    assert emd.tolist() == [auction_host(a, b, EPS)[3] for a, b in zip(want[:3], want[3:])]


def _write_folder(path, rng, count):
    path.mkdir()
    clouds = []
    for i in range(count):
        pts = lidar_like(rng, int(rng.integers(900, 3000)))
        np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1).tofile(str(path / f"{i:04d}.bin"))
        clouds.append(pts)
    return clouds


def test_evaluate_generation_sampling_fps_one_process_and_two_ranks(tmp_path):
    rng = np.random.default_rng(4)
    gen = _write_folder(tmp_path / "gen", rng, 6)
    ref = _write_folder(tmp_path / "ref", rng, 5)
    n, seed = 64, 3
    args = ["generation", str(tmp_path / "gen"), str(tmp_path / "ref"), "--points", str(n), "--seed", str(seed)]
    draw = lambda p, i: np.random.Generator(np.random.PCG64(seed + i))
    fps_cut = lambda cs: _dev([c[np.sort(fps_host(c, n, int(draw(len(c), i).integers(len(c)))))] for i, c in enumerate(cs)])
    rnd_cut = lambda cs: _dev([c[np.sort(draw(len(c), i).choice(len(c), size=n, replace=False))] for i, c in enumerate(cs)])

    one = _run_evaluate(1, args + ["--sampling", "fps"], timeout=300)
    res = json.loads(one)
    assert res["sampling"] == "fps" and res["points"] == n and res["n_gen"] == 6 and res["n_ref"] == 5
    direct = M.generation_metrics(fps_cut(gen), fps_cut(ref))
    assert {k: res[k] for k in direct} == direct

    emd = _run_evaluate(1, args + ["--sampling", "fps", "--emd"], timeout=300)
    res_emd = json.loads(emd)
    direct = M.generation_metrics(fps_cut(gen), fps_cut(ref), emd=True)
    assert {k: res_emd[k] for k in direct} == direct and res_emd["sampling"] == "fps" and res_emd["emd_eps"] == 2.0 ** -7
    assert {k: res_emd[k] for k in res} == res           # --emd works unchanged on top

    # without the flag: today's object, no new key, the random draw
    plain = _run_evaluate(1, args, timeout=300)
    res_plain = json.loads(plain)
    assert set(res_plain) == {"task", "points", "mmd_cd", "cov_cd", "nna_cd", "nna_cd_gen", "nna_cd_ref", "n_gen", "n_ref",
                              "jsd", "mmd"}
    assert set(res) - set(res_plain) == {"sampling"}
    direct = M.generation_metrics(rnd_cut(gen), rnd_cut(ref))
    assert {k: res_plain[k] for k in direct} == direct
    assert res_plain["mmd_cd"] != res["mmd_cd"]          # (the two samplings do pick different points)

    # (only now, after the first launches succeeded) two ranks on this one GPU: byte-identical output
    assert _run_evaluate(2, args + ["--sampling", "fps", "--emd"], timeout=300) == emd
