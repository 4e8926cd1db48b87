"""What stands around the RangeNet++ forward, on the device (rangeldm_amd/csrc/rangenet_post.hip; rangenet.project_scans,
unproject, RangeNet.segment; `evaluate rangenet --projection device --labels-dir`, `evaluate frd --rangenet --projection device`).

Pixels.  The device computes a point's pixel with the same fp32 operations as numpy except for atan2f and asinf, which are the
device's.  Both are accurate to a few ulp; 8 ulp of the [0, 2) intermediate (yaw / pi + 1, and 1 - (pitch + |fov_down|) / fov
lies in [0, 1]) is 8 * 2^-23 = 2^-20, and `* 0.5 * W` carries that to dx = W * 2^-21 (dy = H * 2^-21) in the coordinate that
`floor` sees.  So a point's px (py) may differ from the host's only if the host's fp32 coordinate lies within dx (dy) of an
integer, and the share of points inside that band must itself be at most 0.5 % -- else the band would excuse anything.
Everything after the pixels is exact: given the device's own px, py and depth, rangenet.scatter_host must reproduce proj, mask,
proj_range and proj_idx bit for bit, and given the device's images, rangenet.knn_labels_host the labels.  Nothing is excluded.

Instances.  The unprojection is one of six instances unproject_kernel<S, K> (window S x S, K slots kept): <1, 1>, <3, 9>,
<5, 8> and <7, 8> while knn <= 8, <5, 25> and <7, 49> above.  KNN_PAIRS sits on both sides of that switch and at
knn == search^2, with cutoffs that include 0 ("no cutoff": entries at infinite distance vote); a test derives each pair's
instance from the dispatcher's rule and requires all six.

The stride.  scan_keys_kernel and unproject_kernel give a cloud 128 blocks of 256 threads, which stride over its points in
steps of STRIDE = 32 768.  The `long_cloud` tests project and unproject a ragged batch whose first cloud has about 39 960
points (a KITTI scan has about 120 000), so that threads take a second trip, and hold it to everything the shorter batch is
held to.
"""
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import rangenet as R
from test_generation_metrics import _run_evaluate
from test_rangenet_host import golden_state, load_golden
from test_rangenet_post_host import host_pixels, load_post_golden

pytestmark = pytest.mark.gpu

SIZES = [(64, 1024), (16, 64)]


def _cloud(seed, n):
    pts, rem = R.synthetic_cloud(seed, n=n)
    return np.concatenate([pts, rem[:, None]], 1).astype(np.float32)


STRIDE = 128 * 256                                       # points one trip of the per-point kernels covers: SCAN_BLOCKS_X * 256
_batches = {}


def _downloaded(s):
    names = ("proj", "mask", "proj_range", "proj_idx", "px", "py", "unproj_range", "offsets")
    return {k: getattr(s, k).cpu().numpy() for k in names}


def _ragged_batch(hw):
    """The batch of sizes [20000, 0, 1, 777] projected on the device at hw, downloaded once: (clouds, dict of numpy arrays)."""
    if hw not in _batches:
        big = _cloud(7, 20000)
        clouds = [big, np.zeros((0, 4), np.float32), _cloud(8, 1000)[500:501], _cloud(9, 800)[:777]]
        assert [c.shape[0] for c in clouds][1:] == [0, 1, 777] and 19900 <= clouds[0].shape[0] <= 20000
        s = R.project_scans(clouds, H=hw[0], W=hw[1])
        _batches[hw] = (clouds, _downloaded(s))
    return _batches[hw]


_long_batches = {}


def _long_batch(hw):
    """A batch whose first cloud is longer than one stride, [about 39 960, 0, 777], projected on the device at hw and
    downloaded once: (clouds, the ProjectedScans, dict of numpy arrays)."""
    if hw not in _long_batches:
        clouds = [_cloud(17, 40000), np.zeros((0, 4), np.float32), _cloud(9, 800)[:777]]
        n0 = clouds[0].shape[0]
        print(f"{hw}: clouds of {[c.shape[0] for c in clouds]} points, {n0 - STRIDE} of the first beyond one stride of {STRIDE}")
        assert STRIDE + 5000 < n0 <= 40000 and [c.shape[0] for c in clouds][1:] == [0, 777]
        s = R.project_scans(clouds, H=hw[0], W=hw[1])
        _long_batches[hw] = (clouds, s, _downloaded(s))
    return _long_batches[hw]


def _assert_image_is_scatter_host(cloud, got, b, lo, hi, hw, what):
    H, W = hw
    want = R.scatter_host(got["px"][lo:hi], got["py"][lo:hi], got["unproj_range"][lo:hi], cloud[:, :3], cloud[:, 3], H, W)
    for name, w in zip(("proj", "mask", "proj_range", "proj_idx"), want):
        g = got[name][b]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}"
        bad = int((g != w).sum())
        print(f"{what}: {name}: {bad} of {w.size} values differ")
        assert bad == 0, f"{what}: {name}"


# ---- 1. pixels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES, ids=str)
def test_pixels_equal_the_hosts_outside_a_libm_band(hw):
    _assert_pixels_equal_the_hosts_outside_a_libm_band(*_ragged_batch(hw), hw)


def _assert_pixels_equal_the_hosts_outside_a_libm_band(clouds, got, hw):
    H, W = hw
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).tolist()
    pts = np.concatenate(clouds, 0)[:, :3]
    hx, hy, depth, fx, fy = host_pixels(pts, H, W)
    assert got["unproj_range"].dtype == np.float32
    assert np.array_equal(got["unproj_range"].view(np.uint32), depth.astype(np.float32).view(np.uint32))
    for name, mine, host, f, delta in (("px", got["px"], hx, fx, W * 2.0 ** -21), ("py", got["py"], hy, fy, H * 2.0 ** -21)):
        to_boundary = np.abs(f.astype(np.float64) - np.rint(f.astype(np.float64)))
        share = float((to_boundary <= delta).mean())
        differ = mine != host
        worst = float(to_boundary[differ].max()) if differ.any() else 0.0
        print(f"{H} x {W} {name}: {int(differ.sum())} of {differ.size} differ, the farthest {worst:.3e} from its boundary "
              f"(band {delta:.3e}); {share:.4%} of the points lie inside the band")
        assert share <= 0.005
        assert mine.min() >= 0 and mine.max() < (W if name == "px" else H)
        assert not (differ & (to_boundary > delta)).any()
        assert np.abs(mine[differ].astype(np.int64) - host[differ]).max(initial=0) <= 1


# ---- 2. the image, exact given the pixels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES, ids=str)
def test_image_is_scatter_host_of_the_devices_pixels(hw):
    clouds, got = _ragged_batch(hw)
    off = got["offsets"]
    for b, cloud in enumerate(clouds):
        _assert_image_is_scatter_host(cloud, got, b, off[b], off[b + 1], hw, f"{hw} cloud {b} ({cloud.shape[0]} points)")
    assert (got["proj_idx"][1] == -1).all() and not got["mask"][1].any()         # the empty cloud
    if hw == (16, 64):                                   # about 20 points per pixel: the atomics really contend
        assert np.bincount(got["py"][:off[1]].astype(np.int64) * 64 + got["px"][:off[1]]).mean() > 15


def test_ties_go_to_the_lowest_index_and_point_zero_is_masked():
    hw = (16, 64)
    base = _cloud(11, 3000)
    dup = np.concatenate([base[:600], base[:600], base[600:]], 0)          # 600 points twice: same pixel, same depth
    dup[600:1200, 3] += 1.0                                                # the copies carry another remission
    near = base.copy()
    near[0, :3] = base[1500, :3] * np.float32(0.25)                       # point 0: in point 1500's direction, much nearer
    three = base[:, :3].copy()                                             # a cloud without the remission column
    s = R.project_scans([dup, near, three], H=hw[0], W=hw[1])
    got = {k: getattr(s, k).cpu().numpy() for k in ("proj", "mask", "proj_range", "proj_idx", "px", "py", "unproj_range", "offsets")}
    off = got["offsets"]
    for b, cloud in enumerate((dup, near, np.concatenate([three, np.zeros((three.shape[0], 1), np.float32)], 1))):
        _assert_image_is_scatter_host(cloud, got, b, off[b], off[b + 1], hw, f"cloud {b}")
    idx = got["proj_idx"][0]
    assert not ((idx >= 600) & (idx < 1200)).any() and ((idx >= 0) & (idx < 600)).sum() > 50     # never the copy
    zero = got["proj_idx"][1] == 0
    assert zero.sum() == 1 and got["mask"][1][zero] == 0 and got["proj_range"][1][zero] > 0 and not got["proj"][1][:, zero].any()


def test_a_permutation_gives_the_same_image_and_dropped_points_change_nothing():
    hw = (16, 64)
    base = _cloud(12, 3000)                              # pairwise distinct depths: no ties
    perm = np.concatenate([[0], 1 + np.random.default_rng(0).permutation(base.shape[0] - 1)])    # (point 0 stays: the mask
    bad = np.asarray([[0, 0, 0, 0.5], [np.nan, 1, 1, 0.5], [np.inf, 0, 0, 0.5], [1, -np.inf, 2, 0.5]], np.float32)  # names it)
    withbad = np.concatenate([base[:1000], bad[:2], base[1000:], bad[2:]], 0)
    s = R.project_scans([base, base[perm], withbad], H=hw[0], W=hw[1])
    for name in ("proj", "mask", "proj_range"):
        t = getattr(s, name)
        assert torch.equal(t[0], t[1]) and torch.equal(t[0], t[2]), name
    idx = s.proj_idx.cpu().numpy()
    assert np.array_equal(np.where(idx[1] >= 0, perm[np.maximum(idx[1], 0)], -1), idx[0])
    px, py = s.split(s.px)[2].cpu().numpy(), s.split(s.py)[2].cpu().numpy()
    dropped = np.asarray([1000, 1001, withbad.shape[0] - 2, withbad.shape[0] - 1])
    assert (px[dropped] == -1).all() and (py[dropped] == -1).all()
    keep = np.setdiff1d(np.arange(withbad.shape[0]), dropped)
    assert np.array_equal(px[keep], s.split(s.px)[0].cpu().numpy()) and (px[keep] >= 0).all()
    labels = R.unproject(s, torch.full(tuple(s.mask.shape), 5, dtype=torch.uint8, device="cuda"))
    assert s.split(labels)[2].cpu().numpy()[dropped].tolist() == [0, 0, 0, 0] and int(labels.sum()) == 5 * (labels.numel() - 4)


# ---- 3. back to the points ------------------------------------------------------------------------------------------------
def _blocky(seed, B, H, W):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, R.NUM_CLASSES, (B, (H + 3) // 4, (W + 7) // 8))
    return np.repeat(np.repeat(blocks, 4, 1), 8, 2)[:, :H, :W].astype(np.uint8)


_knn_inputs = {}


def _knn_batch(hw):
    """Two clouds around an empty one, projected on the device; a blocky label image; everything the host needs, downloaded."""
    if hw not in _knn_inputs:
        H, W = hw
        n = int(1.5 * H * W)                             # about a fifth of the pixels stay empty
        clouds = [_cloud(21, n), np.zeros((0, 4), np.float32), _cloud(22, n + 100)]
        s = R.project_scans(clouds, H=H, W=W)
        argmax = torch.from_numpy(_blocky(H, 3, H, W)).cuda()
        host = {k: getattr(s, k).cpu().numpy() for k in ("proj_range", "px", "py", "unproj_range", "offsets")}
        for b in (0, 2):
            lo, hi = host["offsets"][b], host["offsets"][b + 1]
            px, py = host["px"][lo:hi], host["py"][lo:hi]
            assert {0, W - 1} <= set(px.tolist()) and {0, H - 1} <= set(py.tolist())     # every border row and column
            assert (host["proj_range"][b] == -1).mean() > 0.05                              # and empty pixels
        _knn_inputs[hw] = (s, argmax, host)
    return _knn_inputs[hw]


@pytest.mark.parametrize("cutoff", [0.5, 1.0])
@pytest.mark.parametrize("knn", [1, 5])
@pytest.mark.parametrize("search", [3, 5, 7])
@pytest.mark.parametrize("hw", [(8, 32), (16, 64)], ids=str)
def test_knn_labels_equal_the_host_restatement(hw, search, knn, cutoff):
    s, argmax, host = _knn_batch(hw)
    params = {"knn": knn, "search": search, "sigma": 1.0, "cutoff": cutoff}
    got = R.unproject(s, argmax, params)
    assert got.dtype == torch.uint8 and got.shape[0] == host["offsets"][-1]
    got = got.cpu().numpy()
    labels = argmax.cpu().numpy()
    changed = 0
    for b in (0, 2):
        lo, hi = host["offsets"][b], host["offsets"][b + 1]
        want = R.knn_labels_host(host["proj_range"][b], host["unproj_range"][lo:hi], labels[b], host["px"][lo:hi], host["py"][lo:hi],
                                 knn, search, 1.0, cutoff)
        bad = int((got[lo:hi] != want).sum())
        changed += int((want != labels[b][host["py"][lo:hi], host["px"][lo:hi]]).sum())
        print(f"{hw} search {search} knn {knn} cutoff {cutoff} cloud {b}: {bad} of {hi - lo} labels differ")
        assert bad == 0
    assert changed > 0


INSTANCES = {(1, 1), (3, 9), (5, 8), (5, 25), (7, 8), (7, 49)}                  # unproject_kernel<S, K>: window, slots kept
KNN_PAIRS = [(1, 1), (3, 9), (5, 8), (5, 9), (5, 25), (7, 8), (7, 9), (7, 20), (7, 49)]       # (search, knn)


def _instance(search, knn):
    """The dispatcher's rule: a window of 1 or 3 keeps every entry; a window of 5 or 7 keeps 8 slots while knn <= 8 and else
    the whole window."""
    return (search, search * search if search <= 3 or knn > 8 else 8)


def test_the_knn_pairs_reach_every_instance():
    reached = {pair: _instance(*pair) for pair in KNN_PAIRS}
    print(", ".join(f"{pair} -> <{s}, {k}>" for pair, (s, k) in reached.items()))
    assert set(reached.values()) == INSTANCES
    for s in (5, 7):                                     # both sides of the switch, and knn == search^2
        assert {(s, 8), (s, 9), (s, s * s)} <= set(KNN_PAIRS)


@pytest.mark.parametrize("cutoff", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("search,knn", KNN_PAIRS, ids=[f"search{s}-knn{k}" for s, k in KNN_PAIRS])
@pytest.mark.parametrize("hw", [(8, 32), (16, 64)], ids=str)
def test_every_unprojection_instance_equals_the_host_restatement(hw, search, knn, cutoff):
    """Each of the six unproject_kernel instances, on both sides of the knn <= 8 switch and with knn == search^2, where every
    window entry and every padding entry is a candidate; cutoff 0 is "no cutoff", the only mode in which an entry at infinite
    distance (an empty pixel) votes."""
    s, argmax, host = _knn_batch(hw)
    got = R.unproject(s, argmax, {"knn": knn, "search": search, "sigma": 1.0, "cutoff": cutoff}).cpu().numpy()
    labels = argmax.cpu().numpy()
    bad = changed = voters_at_inf = 0
    for b in (0, 2):
        lo, hi = host["offsets"][b], host["offsets"][b + 1]
        px, py = host["px"][lo:hi], host["py"][lo:hi]
        want = R.knn_labels_host(host["proj_range"][b], host["unproj_range"][lo:hi], labels[b], px, py, knn, search, 1.0, cutoff)
        bad += int((got[lo:hi] != want).sum())
        changed += int((want != labels[b][py, px]).sum())
        if cutoff == 0.0 and knn == search * search and search > 1:
            empty = np.pad(host["proj_range"][b] < 0, search // 2)
            window = sum(empty[py + dy, px + dx] for dy in range(search) for dx in range(search)) - empty[py + search // 2, px + search // 2]
            voters_at_inf += int((window > 0).sum())
    print(f"{hw} search {search} knn {knn} cutoff {cutoff}: instance <{_instance(search, knn)[0]}, {_instance(search, knn)[1]}>, {bad} of "
          f"{host['offsets'][-1]} labels differ, {changed} differ from the pixel's own label, {voters_at_inf} points with a voter at infinite distance")
    assert _instance(search, knn) in INSTANCES
    assert bad == 0
    assert changed > 0                                   # (a window of one pixel: class 0 never wins, such a point gets 1)
    if cutoff == 0.0 and knn == search * search and search > 1:
        assert voters_at_inf > 0


# ---- 3b. clouds longer than one stride of the per-point kernels -------------------------------------------------------------
LONG_SIZES = [(16, 64), (64, 1024)]


@pytest.mark.parametrize("hw", LONG_SIZES, ids=str)
def test_long_cloud_pixels_equal_the_hosts_outside_a_libm_band(hw):
    """scan_keys_kernel strides over a cloud in steps of STRIDE points: here the first cloud needs a second trip."""
    clouds, _, got = _long_batch(hw)
    _assert_pixels_equal_the_hosts_outside_a_libm_band(clouds, got, hw)
    H, W = hw
    n0 = clouds[0].shape[0]
    hx, hy, depth, fx, fy = host_pixels(clouds[0][STRIDE:, :3], H, W)
    px, py, r = got["px"][STRIDE:n0], got["py"][STRIDE:n0], got["unproj_range"][STRIDE:n0]
    print(f"{hw}: points {STRIDE} .. {n0 - 1}: {int((px != hx).sum())} px and {int((py != hy).sum())} py differ from the host's")
    assert px.min() >= 0 and px.max() < W and py.min() >= 0 and py.max() < H          # written, every one
    assert np.array_equal(r.view(np.uint32), depth.astype(np.float32).view(np.uint32))
    assert (np.abs(px.astype(np.int64) - hx) <= 1).all() and (np.abs(py.astype(np.int64) - hy) <= 1).all()
    assert len(set(zip(px.tolist(), py.tolist()))) > min(H * W, n0 - STRIDE) // 4                # and they are not one value


@pytest.mark.parametrize("hw", LONG_SIZES, ids=str)
def test_long_cloud_image_is_scatter_host_of_the_devices_pixels(hw):
    clouds, _, got = _long_batch(hw)
    off = got["offsets"]
    for b, cloud in enumerate(clouds):
        _assert_image_is_scatter_host(cloud, got, b, off[b], off[b + 1], hw, f"{hw} cloud {b} ({cloud.shape[0]} points)")
    assert (got["proj_idx"][1] == -1).all() and not got["mask"][1].any()         # the empty cloud
    late = int((got["proj_idx"][0] >= STRIDE).sum())
    print(f"{hw}: {late} of {int((got['proj_idx'][0] >= 0).sum())} pixels are won by a point at index {STRIDE} or beyond")
    assert late > 0 and got["proj_idx"][0].max() < clouds[0].shape[0]


@pytest.mark.parametrize("knn", [None, {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}, {"knn": 20, "search": 7, "sigma": 1.0, "cutoff": 0.0}],
                         ids=["plain", "search5-knn5", "search7-knn20-nocutoff"])
@pytest.mark.parametrize("hw", LONG_SIZES, ids=str)
def test_long_cloud_labels_equal_the_host_restatement(hw, knn):
    """unproject_kernel strides like scan_keys_kernel: every point of the long cloud gets its label, plain and by KNN."""
    clouds, s, host = _long_batch(hw)
    argmax = torch.from_numpy(_blocky(hw[0] + 1, 3, *hw)).cuda()
    labels = argmax.cpu().numpy()
    got = R.unproject(s, argmax, knn).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (host["offsets"][-1],)
    for b in (0, 2):
        lo, hi = host["offsets"][b], host["offsets"][b + 1]
        px, py = host["px"][lo:hi], host["py"][lo:hi]
        own = labels[b][py, px]
        want = own if knn is None else R.knn_labels_host(host["proj_range"][b], host["unproj_range"][lo:hi], labels[b], px, py, **knn)
        bad = got[lo:hi] != want
        print(f"{hw} cloud {b}: {int(bad.sum())} of {hi - lo} labels differ ({int(bad[STRIDE:].sum())} at index {STRIDE} or beyond); "
              f"{int((want != own).sum())} differ from the pixel's own label")
        assert not bad.any()
        assert knn is None or (want != own).any()
        if b == 0:
            assert len(set(want[STRIDE:].tolist())) > 1                           # the late points carry labels worth comparing


@pytest.mark.parametrize("i", [0, 1])
def test_knn_labels_equal_the_reference_golden(i):
    g = load_post_golden()
    H, W = (int(v) for v in g[f"c{i}_hw"])
    n = g[f"c{i}_points"].shape[0]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    s = R.ProjectedScans(proj_range=dev(g[f"c{i}_proj_range"][None], torch.float32), px=dev(g[f"c{i}_proj_x"], torch.int32),
                         py=dev(g[f"c{i}_proj_y"], torch.int32), unproj_range=dev(g[f"c{i}_unproj_range"], torch.float32),
                         offsets=dev(np.asarray([0, n]), torch.int32), lengths=[n])
    argmax = dev(g[f"c{i}_argmax"][None], torch.uint8)
    for j, (knn, search, sigma, cutoff) in enumerate(g["params"]):
        got = R.unproject(s, argmax, {"knn": int(knn), "search": int(search), "sigma": float(sigma), "cutoff": float(cutoff)}).cpu().numpy()
        bad = int((got != g[f"c{i}_knn{j}"]).sum())
        print(f"case {i} params {j}: {bad} of {n} labels differ from the reference's KNN")
        assert bad == 0
    plain = R.unproject(s, argmax).cpu().numpy()
    assert np.array_equal(plain, g[f"c{i}_argmax"][g[f"c{i}_proj_y"], g[f"c{i}_proj_x"]])


def test_plain_unprojection_and_refused_parameters():
    s, argmax, host = _knn_batch((16, 64))
    got = R.unproject(s, argmax).cpu().numpy()
    labels = argmax.cpu().numpy()
    for b in (0, 2):
        lo, hi = host["offsets"][b], host["offsets"][b + 1]
        assert np.array_equal(got[lo:hi], labels[b][host["py"][lo:hi], host["px"][lo:hi]])
    one = {"knn": 1, "search": 1, "sigma": 1.0, "cutoff": 1.0}                # the window is the point's own pixel
    got1 = R.unproject(s, argmax, one).cpu().numpy()
    for b in (0, 2):
        lo, hi = host["offsets"][b], host["offsets"][b + 1]
        assert np.array_equal(got1[lo:hi], R.knn_labels_host(host["proj_range"][b], host["unproj_range"][lo:hi], labels[b],
                                                              host["px"][lo:hi], host["py"][lo:hi], **one))
    for bad in ({"search": 4}, {"search": 9}, {"search": 1, "knn": 2}, {"knn": 26}, {"search": 3, "knn": 10}, {"cutoff": -1.0}):
        with pytest.raises(RuntimeError, match="rldm_rangenet_unproject"):
            R.unproject(s, argmax, {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0, **bad})
    with pytest.raises(ValueError):
        R.unproject(s, argmax[:2])
    assert np.array_equal(R.unproject(s, argmax).cpu().numpy(), got)           # a refused call leaves nothing behind


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn", [None, {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}], ids=["plain", "knn"])
def test_segment_is_projection_forward_and_unprojection(knn):
    H, W = 8, 64
    net = R.RangeNet(golden_state(21))
    clouds = [_cloud(31, 900), _cloud(32, 700)[:, :3], _cloud(33, 1200)]
    got = net.segment(clouds, knn=knn, H=H, W=W)
    s = R.project_scans(clouds, H=H, W=W)
    argmax, _ = net.infer(s.proj)
    argmax = argmax.cpu().numpy()
    assert len(got) == 3
    print(f"{len(set(np.concatenate(got).tolist()))} distinct labels over {sum(map(len, got))} points")
    for b, (lab, px, py, r) in enumerate(zip(got, s.split(s.px), s.split(s.py), s.split(s.unproj_range))):
        px, py, r = px.cpu().numpy(), py.cpu().numpy(), r.cpu().numpy()
        if knn is None:
            want = argmax[b][py, px]
        else:
            want = R.knn_labels_host(s.proj_range[b].cpu().numpy(), r, argmax[b], px, py, nclasses=R.NUM_CLASSES, **knn)
        assert lab.dtype == np.uint8 and lab.shape == (clouds[b].shape[0],) and np.array_equal(lab, want)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """A DarkNet21 model folder, two folders of two seeded clouds each, and `evaluate rangenet --projection device` over both
    (folder a with --labels-dir --knn): (root, clouds of a, the JSON lines)."""
    root = tmp_path_factory.mktemp("rangenet_post")
    g = load_golden()
    arch = R.synthetic_arch(21)
    R.save_pretrained(str(root / "model"), arch, *R.synthetic_state(arch, int(g["seed"]), R.bn_stats_from_arrays(21, g["bn21_mean"], g["bn21_var"]),
                                                                    head_bias_std=float(g["head_bias_std"])))
    clouds = {}
    for name, base in (("a", 300), ("b", 400)):
        (root / name).mkdir()
        clouds[name] = [_cloud(base + i, 6000 + 1000 * i) for i in range(2)]
        for i, c in enumerate(clouds[name]):
            c.tofile(str(root / name / f"{i:04d}.bin"))
    outs = {}
    for name in ("a", "b"):
        args = ["rangenet", "--model", str(root / "model"), "--dump", str(root / name), "--frd-dir", str(root / f"frd_{name}"),
                "--output-dir", str(root / f"seg_{name}"), "--projection", "device"]
        if name == "a":
            args += ["--labels-dir", str(root / "labels_a"), "--knn"]
        outs[name] = _run_evaluate(1, args, timeout=300)
    return root, clouds["a"], outs


def test_evaluate_rangenet_writes_per_point_labels(driver, tmp_path):
    root, clouds, outs = driver
    assert json.loads(outs["a"]) == {"task": "rangenet", "files": 2, "layers": 21, "projection": "device", "labels": "knn"}
    assert json.loads(outs["b"]) == {"task": "rangenet", "files": 2, "layers": 21, "projection": "device"}
    arch, sds = R.load_pretrained(str(root / "model"))
    want = R.RangeNet.from_state(arch, *sds).segment(clouds, knn=R.knn_params(arch))
    two = _run_evaluate(2, ["rangenet", "--model", str(root / "model"), "--dump", str(root / "a"), "--frd-dir", str(tmp_path / "frd"),
                            "--output-dir", str(tmp_path / "seg"), "--projection", "device", "--labels-dir", str(tmp_path / "labels"),
                            "--knn"], timeout=300)
    assert two == outs["a"]
    for i, cloud in enumerate(clouds):
        raw = (root / "labels_a" / f"{i}.label").read_bytes()
        lab = np.frombuffer(raw, dtype=np.uint32)
        assert lab.shape == (cloud.shape[0],) and np.array_equal(lab, want[i].astype(np.uint32))
        assert (tmp_path / "labels" / f"{i}.label").read_bytes() == raw
        assert (tmp_path / "frd" / f"{i}.npy").read_bytes() == (root / "frd_a" / f"{i}.npy").read_bytes()


def test_evaluate_frd_with_device_projection_equals_frd_of_its_dumps(driver):
    root, _, _ = driver
    dumps = _run_evaluate(1, ["frd", str(root / "frd_a"), str(root / "frd_b")], timeout=300)
    args = ["frd", "--rangenet", str(root / "model"), str(root / "a"), str(root / "b"), "--projection", "device"]
    direct = _run_evaluate(1, args, timeout=300)
    assert _run_evaluate(2, args, timeout=300) == direct
    res = json.loads(direct)
    assert "projection" not in json.loads(dumps) and res.pop("projection") == "device"
    assert json.dumps(res, sort_keys=True) == dumps      # byte for byte but for the key that names the projection
    assert res["n1"] == 2 and res["n2"] == 2 and res["frd"] > 0
