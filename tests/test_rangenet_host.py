"""RangeNet++ on the host (rangeldm_amd.rangenet): forward_host against the reference network, project_scan against the
reference's LaserScan, segmentation_scores against sklearn, the refusals, the transposed conv's parity identity and the new
sub-commands' argument checks.  Nothing here needs a GPU.

tests/golden/rangenet.npz is written by tools/make_rangenet_golden.py from the reference's own modules on CPU fp32 (its
docstring lists the keys).  The segmentation cases in it are sklearn.metrics.jaccard_score(average="weighted") results (sklearn
imports where the golden is made), plus one case small enough to check by hand below.

FWD_TOL.  forward_host and the reference are the same fp32 arithmetic in different groupings (BatchNorm folded into one
multiply-add against torch's batch_norm; the transposed conv is torch's in both), so they differ by torch-CPU rounding noise.
Measured where the golden was made: rel-L2 1.70e-06 (DarkNet21 features) / 6.1e-07 (logits), 1.68e-06 / 6.0e-07 (DarkNet53).
The gate is 10 x the largest.
"""
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import rangenet as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangenet.npz")
FULL_SEED = 53                                           # the seeded scan of the full-size case (synthetic_cloud)
FWD_MEASURED = 1.7e-06                                   # the largest rel-L2 of forward_host to the golden, see above
FWD_TOL = 10 * FWD_MEASURED

_golden = None


def load_golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


_states = {}


def golden_state(layers, g=None):
    """The synthetic network of the golden: seeded weights, the recorded BatchNorm statistics, the recorded spread of the head's class biases."""
    g = g or load_golden()
    if layers not in _states:
        arch = R.synthetic_arch(layers)
        stats = R.bn_stats_from_arrays(layers, g[f"bn{layers}_mean"], g[f"bn{layers}_var"])
        _states[layers] = R.fold_state(arch, *R.synthetic_state(arch, int(g["seed"]), stats, head_bias_std=float(g["head_bias_std"])))
    return _states[layers]


def small_case(layers):
    """(state, input (2, 5, 8, 64), reference features (2, 32, 8, 64), reference logits (2, 20, 8, 64))"""
    g = load_golden()
    t = lambda k: torch.from_numpy(g[f"small{layers}_{k}"])
    return golden_state(layers), t("x"), t("feat"), t("logits")


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("layers", [21, 53])
def test_forward_host_matches_the_reference(layers):
    state, x, feat_ref, logits_ref = small_case(layers)
    feat, logits, rms = R.forward_host(state, x, return_rms=True)
    ef, el = _rel_l2(feat, feat_ref), _rel_l2(logits, logits_ref)
    print(f"DarkNet{layers}: features rel-L2 {ef:.2e}, logits {el:.2e} (gate {FWD_TOL:.1e}); layer RMS in [{min(rms):.3f}, {max(rms):.3f}]")
    assert tuple(feat.shape) == (2, 32, 8, 64) and tuple(logits.shape) == (2, 20, 8, 64)
    assert ef <= FWD_TOL and el <= FWD_TOL
    # the calibrated BatchNorm statistics keep every layer's output in a sane range
    assert len(rms) == len(state["specs"]) and 0.1 <= min(rms) and max(rms) <= 10.0


def test_emulation_rounds_where_the_kernel_rounds():
    """bf16=True differs from fp32 by rounding noise only, and its stored activations are bf16 values."""
    state, x, feat_ref, _ = small_case(21)
    feat, _ = R.forward_host(state, x, bf16=True)
    assert 1e-4 < _rel_l2(feat, feat_ref) < 0.1
    s = state["specs"][0]
    out, v = R.layer_host(s["kind"], x, s["w"], s["scale"], s["shift"], True, bf16=True)
    assert torch.equal(out, v.to(torch.bfloat16).to(torch.float32)) and not torch.equal(out, v)


def test_layer_lists_agree():
    for layers, n in ((21, 36), (53, 68)):
        specs = R.layer_specs(layers)
        assert len(specs) == n and len(R.bn_names(layers)) == n - 1
        assert (specs[-1]["cin"], specs[-1]["cout"], specs[-1]["leaky"]) == (32, 20, False)
        for a, b in zip(specs[:-1], specs[1:]):
            assert a["cout"] == b["cin"]


@pytest.mark.parametrize("case", [0, 1])
def test_project_scan_matches_the_reference(case):
    g = load_golden()
    pts, rem = g[f"proj{case}_points"], g[f"proj{case}_remission"]
    H, W = g[f"proj{case}_out"].shape[1:]
    proj, mask = R.project_scan(pts, rem if case == 0 else None, H=H, W=W)
    assert proj.dtype == np.float32 and proj.shape == (5, H, W)
    assert np.array_equal(mask, g[f"proj{case}_mask"]) and np.array_equal(proj, g[f"proj{case}_out"])
    # point 0 wins a pixel (it is the nearest there) and the reference's `proj_idx > 0` drops it
    assert 0.3 < mask.mean() < 1.0


def test_project_scan_drops_point_zero():
    pts = np.array([[5.0, 0.0, -0.5], [0.0, 7.0, -0.5], [-6.0, 1.0, -1.0]], np.float32)
    proj, mask = R.project_scan(pts, np.ones(3, np.float32), H=8, W=16)
    assert int(mask.sum()) == 2 and not proj[:, mask == 0].any()
    with pytest.raises(ValueError):
        R.project_scan(np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        R.project_scan(pts, np.ones(2, np.float32))


def test_segmentation_scores_match_sklearn():
    g = load_golden()
    n = int(g["seg_cases"])
    assert n >= 3
    for i in range(n):
        got = R.segmentation_scores(torch.from_numpy(g[f"seg{i}_pred"]), torch.from_numpy(g[f"seg{i}_target"]))
        assert abs(got["iou"] - float(g[f"seg{i}_iou"])) <= 1e-15 and abs(got["accuracy"] - float(g[f"seg{i}_accuracy"])) <= 1e-15


def test_segmentation_scores_by_hand():
    # target 0 1 1 2 / pred 0 1 2 2: class 0 IoU 1 (support 1), class 1 1/2 (support 2), class 2 1/2 (support 1)
    got = R.segmentation_scores(torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 1, 2]))
    assert got == {"accuracy": 0.75, "iou": (1.0 + 2 * 0.5 + 0.5) / 4}
    # a class that only the prediction holds has weight 0 but still costs the classes it was taken from
    got = R.segmentation_scores(torch.tensor([3, 3]), torch.tensor([1, 1]))
    assert got == {"accuracy": 0.0, "iou": 0.0}
    cm = R.confusion_matrix(torch.tensor([[0, 19]]), torch.tensor([[0, 0]]))
    assert cm.dtype == torch.int64 and cm.shape == (20, 20) and int(cm[0, 19]) == 1 and int(cm.sum()) == 2
    with pytest.raises(ValueError):
        R.segmentation_scores(torch.tensor([0, 20]), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        R.segmentation_scores(torch.tensor([0, 1, 2]), torch.tensor([0, 1]))


def _arch(**edits):
    arch = R.synthetic_arch(53)
    for path, value in edits.items():
        node = arch
        keys = path.split("__")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = value
    return arch


@pytest.mark.parametrize("edit", [{"backbone__name": "squeezeseg"}, {"decoder__name": "squeezesegV2"}, {"post__CRF__use": True},
                                  {"post__KNN__use": True}, {"backbone__OS": 16}, {"backbone__extra__layers": 19},
                                  {"backbone__input_depth__xyz": False}], ids=str)
def test_what_is_not_built_is_refused(edit, tmp_path):
    arch = _arch(**edit)
    with pytest.raises(NotImplementedError):
        R.check_arch(arch)
    with pytest.raises(NotImplementedError):
        R.fold_state(arch, {}, {}, {})
    # from_pretrained refuses on the yaml alone, before a weight file is read (there is none here) and before any GPU work
    import yaml
    (tmp_path / "arch_cfg.yaml").write_text(yaml.safe_dump(arch))
    with pytest.raises(NotImplementedError):
        R.RangeNet.from_pretrained(str(tmp_path))


def test_fold_state_checks_names_and_shapes():
    arch = R.synthetic_arch(21)
    b, d, h = R.synthetic_state(arch, 1)
    assert R.check_arch(arch) == 21
    bad = dict(b)
    del bad["enc3.residual_1.bn2.running_var"]
    with pytest.raises(KeyError):
        R.fold_state(arch, bad, d, h)
    bad = dict(d)
    bad["dec5.upconv.weight"] = bad["dec5.upconv.weight"].permute(1, 0, 2, 3).contiguous()
    with pytest.raises(ValueError):
        R.fold_state(arch, b, bad, h)
    # BatchNorm and the transposed conv's bias fold into one fp32 multiply-add
    st = R.fold_state(arch, b, d, h)
    up = next(s for s in st["specs"] if s["kind"] == R.KIND_UPCONV)
    scale = d["dec5.bn.weight"] / torch.sqrt(d["dec5.bn.running_var"] + 1e-5)
    assert torch.equal(up["scale"], scale)
    assert torch.equal(up["shift"], d["dec5.bn.bias"] - d["dec5.bn.running_mean"] * scale + d["dec5.upconv.bias"] * scale)


@pytest.mark.parametrize("W", [1, 2, 17])
def test_transposed_conv_parity_identity_is_exact(W):
    rng = np.random.default_rng(W)
    x = torch.from_numpy(rng.integers(-4, 5, (2, 6, 3, W)).astype(np.float32))
    w = torch.from_numpy(rng.integers(-2, 3, (6, 5, 1, 4)).astype(np.float32))
    want = torch.nn.functional.conv_transpose2d(x, w, stride=(1, 2), padding=(0, 1))
    assert tuple(want.shape) == (2, 5, 3, 2 * W) and torch.equal(R.upconv_by_parity(x, w), want)


def test_kernel_weight_layout():
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    kw = R.kernel_weight(R.KIND_3X3, w)
    assert kw.shape == (2, 9, 3) and kw[1, 5, 2] == float(w[1, 2, 1, 2])         # tap = 3 ky + kx
    u = torch.arange(3 * 2 * 4, dtype=torch.float32).reshape(3, 2, 1, 4)
    ku = R.kernel_weight(R.KIND_UPCONV, u)
    assert ku.shape == (2, 4, 3) and ku[1, 3, 2] == float(u[2, 1, 0, 3])


def test_new_subcommands_check_their_arguments_before_reading_files(tmp_path):
    from rangeldm_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["rangenet", "--model", "m", "--dump", "d", "--frd-dir", "f", "--output-dir", "o", "--batch-size", "0"])
    with pytest.raises(ValueError, match="batch"):
        E.check_rangenet_args(a)
    same = str(tmp_path / "x")
    a = ap.parse_args(["rangenet", "--model", "m", "--dump", same, "--frd-dir", same, "--output-dir", "o"])
    with pytest.raises(ValueError, match="--frd-dir"):
        E.check_rangenet_args(a)
    E.check_rangenet_args(ap.parse_args(["rangenet", "--model", "m", "--dump", "d", "--frd-dir", "f", "--output-dir", "o"]))
    for missing in (["--dump", "d", "--frd-dir", "f", "--output-dir", "o"], ["--model", "m", "--frd-dir", "f", "--output-dir", "o"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["rangenet"] + missing)
    # frd --rangenet works on whole feature maps: other --total / --count values belong to dumped test folders
    a = ap.parse_args(["frd", "--rangenet", "m", "c1", "c2", "--total", "1000"])
    with pytest.raises(ValueError, match="--total"):
        E.check_frd_args(a)
    a = ap.parse_args(["frd", "--rangenet", "m", "c1", "c2", "--limit", "1"])
    with pytest.raises(ValueError, match="--limit"):
        E.check_frd_args(a)
    E.check_frd_args(ap.parse_args(["frd", "--rangenet", "m", "c1", "c2"]))
    assert ap.parse_args(["frd", "c1", "c2"]).rangenet is None
    a = ap.parse_args(["segmentation", "r", "t", "--classes", "0"])
    with pytest.raises(ValueError, match="--classes"):
        E.check_segmentation_args(a)
    a = ap.parse_args(["segmentation", "r", "t"])
    assert a.classes == 20 and E.check_segmentation_args(a) is None
