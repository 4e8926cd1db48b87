"""The host restatements of what stands around the RangeNet++ forward (rangeldm_amd.rangenet: scatter_host, knn_weights,
knn_labels_host) against tests/golden/rangenet_post.npz, which tools/make_rangenet_post_golden.py recorded from the reference's
LaserScan and postproc/KNN.py on tie-free clouds (the tool asserts that): every comparison is exact, nothing is excluded.
"""
import os

import numpy as np
import pytest

from rangeldm_amd import rangenet as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangenet_post.npz")
_golden = None


def load_post_golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def golden_cases():
    g = load_post_golden()
    return range(int(g["cases"])), [tuple(p) for p in g["params"]]


def host_pixels(points, H, W, fov_up=3.0, fov_down=-25.0):
    """(px, py, depth, fx, fy) of rangenet.project_scan's lines before the sort: the integer pixels, and the fp32 coordinates
    just before `floor`."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    fov_up_r, fov_down_r = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = abs(fov_down_r) + abs(fov_up_r)
    depth = np.linalg.norm(points, 2, axis=1)
    yaw = -np.arctan2(points[:, 1], points[:, 0])
    pitch_ = np.arcsin(points[:, 2] / depth)
    fx = 0.5 * (yaw / np.pi + 1.0)
    fy = 1.0 - (pitch_ + abs(fov_down_r)) / fov
    fx *= W
    fy *= H
    px = np.maximum(0, np.minimum(W - 1, np.floor(fx))).astype(np.int32)
    py = np.maximum(0, np.minimum(H - 1, np.floor(fy))).astype(np.int32)
    return px, py, depth, fx, fy


# ---- the golden ------------------------------------------------------------------------------------------------------------
def test_knn_weights_are_the_references_bits():
    g = load_post_golden()
    for j, (knn, search, sigma, cutoff) in enumerate(golden_cases()[1]):
        w = R.knn_weights(int(search), sigma)
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), g[f"w{j}"].view(np.uint32))


@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("i", [0, 1])
def test_knn_labels_host_equals_the_reference(i, j):
    g = load_post_golden()
    knn, search, sigma, cutoff = g["params"][j]
    got = R.knn_labels_host(g[f"c{i}_proj_range"], g[f"c{i}_unproj_range"], g[f"c{i}_argmax"], g[f"c{i}_proj_x"], g[f"c{i}_proj_y"],
                            int(knn), int(search), float(sigma), float(cutoff), R.NUM_CLASSES)
    want = g[f"c{i}_knn{j}"]
    plain = g[f"c{i}_argmax"][g[f"c{i}_proj_y"], g[f"c{i}_proj_x"]]
    print(f"case {i}, params {j}: {int((got != want).sum())} of {want.size} labels differ; KNN changes {float((want != plain).mean()):.1%}")
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert (want != plain).mean() > 0.02                 # the comparison is about more than the plain unprojection


@pytest.mark.parametrize("i", [0, 1])
def test_scatter_host_reproduces_project_scan_and_the_reference(i):
    g = load_post_golden()
    H, W = (int(v) for v in g[f"c{i}_hw"])
    pts, rem = g[f"c{i}_points"], g[f"c{i}_remission"]
    px, py, depth = g[f"c{i}_proj_x"], g[f"c{i}_proj_y"], g[f"c{i}_unproj_range"]
    hx, hy, hd, _, _ = host_pixels(pts, H, W)
    assert np.array_equal(hx, px) and np.array_equal(hy, py) and np.array_equal(hd, depth)       # (this restatement, too)
    proj, mask, proj_range, proj_idx = R.scatter_host(px, py, depth, pts, rem, H, W)
    want_proj, want_mask = R.project_scan(pts, rem, H=H, W=W)
    assert np.array_equal(proj, want_proj) and np.array_equal(mask, want_mask)
    assert np.array_equal(proj_range, g[f"c{i}_proj_range"])
    assert proj.dtype == np.float32 and mask.dtype == np.float32 and proj_idx.dtype == np.int32
    assert np.array_equal(mask, (proj_idx > 0).astype(np.float32)) and (proj_idx == -1).any()


# ---- the pixel rule by hand ------------------------------------------------------------------------------------------------
def test_equal_depths_go_to_the_lower_index_and_dropped_points_take_no_part():
    # points 1 and 2: one pixel, one depth, different remission; point 3 farther in the same pixel; point 4 dropped
    pts = np.asarray([[5, 0, 0], [0, 3, 0], [0, 3, 0], [0, 4, 0], [0, 0, 0]], np.float32)
    rem = np.asarray([0.1, 0.2, 0.3, 0.4, 0.5], np.float32)
    px = np.asarray([0, 2, 2, 2, -1])
    py = np.asarray([0, 1, 1, 1, -1])
    depth = np.asarray([5, 3, 3, 4, 0], np.float32)
    proj, mask, proj_range, proj_idx = R.scatter_host(px, py, depth, pts, rem, H=2, W=4, means=(0,) * 5, stds=(1,) * 5)
    assert proj_idx[1, 2] == 1 and proj[4, 1, 2] == np.float32(0.2) and proj_range[1, 2] == 3
    for order in ([2, 1], [1, 2]):                       # whatever order the rows come in: the index decides
        sw = np.asarray([0] + order + [3, 4])
        _, _, _, idx = R.scatter_host(px[sw], py[sw], depth[sw], pts[sw], rem[sw], H=2, W=4)
        assert idx[1, 2] == 1
    # point 0 wins pixel (0, 0): in the index image, masked out of the input (the reference's `proj_idx > 0`)
    assert proj_idx[0, 0] == 0 and mask[0, 0] == 0 and proj_range[0, 0] == 5 and not proj[:, 0, 0].any()
    assert int((proj_idx >= 0).sum()) == 2 and mask.sum() == 1


# ---- KNN by hand -----------------------------------------------------------------------------------------------------------
def _knn_one(proj_range, argmax, x, y, r, **kw):
    p = {"knn": 5, "search": 3, "sigma": 1.0, "cutoff": 1.0, **kw}
    return int(R.knn_labels_host(proj_range, np.asarray([r], np.float32), argmax, np.asarray([x]), np.asarray([y]),
                                 p["knn"], p["search"], p["sigma"], p["cutoff"], R.NUM_CLASSES)[0])


def test_knn_corner_sees_padding_as_range_zero_label_zero():
    # corner (0, 0) of an 8 x 32 image, the point 0.5 m away: the five padded entries (range 0) lie at |0 - 0.5| * w < cutoff
    # and vote for class 0, which never wins; the in-image neighbours are 10 m off, beyond the cutoff; the centre votes 7
    rng = np.full((8, 32), 10.0, np.float32)
    rng[0, 0] = 0.5
    lab = np.full((8, 32), 3, np.uint8)
    lab[0, 0] = 7
    assert _knn_one(rng, lab, 0, 0, 0.5, knn=9) == 7
    # the nearest 5 are the centre (distance 0) and four padded zeros: one vote for 7 still beats any number for class 0
    assert _knn_one(rng, lab, 0, 0, 0.5, knn=5) == 7
    # without the padding rule (neighbours at infinity or wrapped) the in-cutoff set would differ: move the point to 10 m and the
    # three in-image neighbours vote 3 against the centre's 7
    assert _knn_one(rng, lab, 0, 0, 10.0, knn=9, cutoff=20.0) == 3


def test_knn_without_votes_gives_class_one():
    # every neighbour is empty (-1 -> +inf) and the centre's own label is 0: nobody votes
    rng = np.full((8, 32), -1.0, np.float32)
    rng[4, 10] = 6.0
    lab = np.full((8, 32), 9, np.uint8)
    lab[4, 10] = 0
    assert _knn_one(rng, lab, 10, 4, 6.0) == 1
    # and a dropped point gets 0
    got = R.knn_labels_host(rng, np.asarray([6.0, 0.0], np.float32), lab, np.asarray([10, -1]), np.asarray([4, -1]), 5, 3, 1.0, 1.0)
    assert got.tolist() == [1, 0]


def test_knn_votes_for_class_zero_never_win():
    # four neighbours and the centre say 0, one says 12: 12 wins; two classes tie at one vote each: the lower wins
    rng = np.full((8, 32), -1.0, np.float32)
    lab = np.zeros((8, 32), np.uint8)
    rng[3:6, 9:12] = 6.0
    lab[3, 9] = 12
    assert _knn_one(rng, lab, 10, 4, 6.0, knn=9) == 12
    lab[5, 11] = 4
    assert _knn_one(rng, lab, 10, 4, 6.0, knn=9) == 4
    # equal distances: the stable sort keeps window order, so with knn = 2 entries k = 0 (label 12) and k = 1 (label 0) are in
    rng[...] = 6.0
    assert _knn_one(rng, lab, 10, 4, 6.0, knn=2) == 12


def test_knn_params_are_checked():
    arch = R.synthetic_arch(21)
    assert R.knn_params(arch) == {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
    for bad in ({"search": 4}, {"search": 9}, {"knn": 26}, {"knn": 0}, {"sigma": 0.0}, {"cutoff": -1.0}):
        with pytest.raises(ValueError):
            R.check_knn({"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0, **bad})
    with pytest.raises(ValueError):
        R.knn_params({"post": {"KNN": {"use": False, "params": False}}})
    arch["post"]["KNN"]["use"] = True                    # asked for explicitly, never through the arch_cfg
    with pytest.raises(NotImplementedError):
        R.check_arch(arch)


def test_pack_clouds_checks_shapes():
    a, b = np.zeros((3, 4), np.float32), np.ones((2, 3), np.float32)
    with pytest.raises(ValueError):
        R.pack_clouds([a, np.zeros((2, 5), np.float32)], device="cpu")
    with pytest.raises(ValueError):
        R.pack_clouds(np.zeros((5, 4), np.float32), [2, 2], device="cpu")
    packed, lengths = R.pack_clouds([a, b], device="cpu")
    assert lengths == [3, 2] and tuple(packed.shape) == (5, 4) and packed[3:, 3].abs().sum() == 0 and packed[3:, :3].min() == 1


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_projection_and_label_arguments_are_checked_before_files_are_read():
    from rangeldm_amd import evaluate as E
    ap = E.build_parser()
    base = ["rangenet", "--model", "m", "--dump", "d", "--frd-dir", "f", "--output-dir", "o"]
    plain = ap.parse_args(base)
    assert plain.projection == "host" and plain.labels_dir is None and plain.knn is False
    assert vars(ap.parse_args(base + ["--projection", "host"])) == vars(plain)
    E.check_rangenet_args(plain)
    E.check_rangenet_args(ap.parse_args(base + ["--projection", "device", "--labels-dir", "l", "--knn"]))
    for extra, word in ((["--knn"], "--labels-dir"), (["--projection", "device", "--knn"], "--labels-dir"),
                        (["--labels-dir", "l"], "--projection device"), (["--projection", "device", "--labels-dir", "d"], "--dump")):
        with pytest.raises(ValueError, match=word):
            E.check_rangenet_args(ap.parse_args(base + extra))
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--projection", "gpu"])
    frd = ap.parse_args(["frd", "a", "b"])
    assert frd.projection == "host" and vars(ap.parse_args(["frd", "a", "b", "--projection", "host"])) == vars(frd)
    E.check_frd_args(frd)
    E.check_frd_args(ap.parse_args(["frd", "a", "b", "--rangenet", "m", "--projection", "device"]))
    with pytest.raises(ValueError, match="--rangenet"):
        E.check_frd_args(ap.parse_args(["frd", "a", "b", "--projection", "device"]))


def test_label_settings_read_the_model_folder(tmp_path):
    import yaml
    from rangeldm_amd import evaluate as E
    arch = R.synthetic_arch(21)
    with open(tmp_path / "arch_cfg.yaml", "w") as f:
        yaml.safe_dump(arch, f)
    assert E.label_settings(str(tmp_path), False) == (None, None)
    knn, table = E.label_settings(str(tmp_path), True)
    assert knn == {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0} and table is None
    with open(tmp_path / "data_cfg.yaml", "w") as f:
        yaml.safe_dump({"learning_map_inv": {0: 0, 1: 10, 2: 11, 19: 81}}, f)
    _, table = E.label_settings(str(tmp_path), False)
    assert table.dtype == np.uint32 and table.shape == (20,) and table[[0, 1, 2, 19, 5]].tolist() == [0, 10, 11, 81, 0]
