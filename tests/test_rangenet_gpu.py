"""RangeNet++ inference on the device (rangeldm_amd/csrc/rangenet.hip; rangeldm_amd.rangenet; `evaluate rangenet`,
`evaluate frd --rangenet`, `evaluate segmentation`).

Layers.  On integer-valued operands (inputs in [-4, 4], weights in [-2, 2], scale in {0.5, 1, 2}, integer shift and addends)
every product and every partial sum is an integer below 2^24 (at most 9 taps x 1024 channels x 8), so whatever order the MFMA
adds in, the accumulator is exact; the epilogue after it is one fp32 operation per step, so rldm_rangenet_layer must equal
rangenet.layer_host bit for bit, the single fp32 multiply by 0.1f and the final rounding to bf16 included.

Network.  The bound on the device's distance to the reference golden is 2 x the distance of forward_host(bf16=True) -- the
rounding the design accepts, restated in torch on the CPU -- to the same golden: measured without the code under test (here for
the small cases, when the golden was made for the full-size one).  The factor 2 covers the accumulation order of the MFMA tiles
against torch's sums.  Every test prints its figures before it asserts.
"""
import json
import zlib

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M
from rangeldm_amd import rangenet as R
from test_generation_metrics import _run_evaluate
from test_rangenet_host import FULL_SEED, golden_state, load_golden, small_case

pytestmark = pytest.mark.gpu

KINDS = {"1x1": R.KIND_1X1, "3x3": R.KIND_3X3, "3x3s2": R.KIND_3X3_S2, "upconv": R.KIND_UPCONV}


def _operands(kind, B, H, W, cin, cout, seed, add0=False, add1=False):
    rng = np.random.default_rng(seed)
    Wout = (W - 1) // 2 + 1 if kind == R.KIND_3X3_S2 else 2 * W if kind == R.KIND_UPCONV else W
    wshape = (cin, cout, 1, 4) if kind == R.KIND_UPCONV else (cout, cin) + ((1, 1) if kind == R.KIND_1X1 else (3, 3))
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    op = {"x": t(rng.integers(-4, 5, (B, cin, H, W))), "w": t(rng.integers(-2, 3, wshape)),
          "scale": t(rng.choice([0.5, 1.0, 2.0], cout)), "shift": t(rng.integers(-6, 7, cout)),
          "add0": t(rng.integers(-8, 9, (B, cout, H, Wout))) if add0 else None,
          "add1": t(rng.integers(-8, 9, (B, cout, H, Wout))) if add1 else None}
    return op


def _device_layer(kind, op, leaky, **kw):
    cin = op["x"].shape[1]
    cout = op["scale"].numel()
    dev = lambda a: R.to_device_layout(a) if a is not None else None
    return R.run_layer(kind, R.to_device_layout(op["x"]), R.pack_weights(kind, op["w"]), op["scale"], op["shift"], cin, cout,
                       leaky=leaky, add0=dev(op["add0"]), add1=dev(op["add1"]), want_f32=True, **kw)


def _assert_layer_exact(kind, op, leaky, what):
    got = _device_layer(kind, op, leaky)
    want_out, want_v = R.layer_host(kind, op["x"], op["w"], op["scale"], op["shift"], leaky, op["add0"], op["add1"], bf16=True)
    cout = want_v.shape[1]
    out = R.from_device_layout(got["out"], cout)
    f32 = got["f32"].cpu()
    assert tuple(out.shape) == tuple(want_out.shape), what
    bad_out, bad_v = int((out != want_out).sum()), int((f32 != want_v).sum())
    print(f"{what}: {bad_out} bf16 and {bad_v} fp32 values of {want_v.numel()} differ")
    assert bad_v == 0 and bad_out == 0, what
    pad = got["out"][..., cout:]
    assert pad.numel() == 0 or not bool(pad.to(torch.float32).abs().max() > 0), f"{what}: pad channels are not zero"


# ---- 1. every layer instance, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [33, 34, 66, 130])
@pytest.mark.parametrize("kind", list(KINDS))
def test_layer_is_exact_at_every_edge(kind, W):
    """odd widths, one past a tile, stride-2 edges; rows 1, 3, 5 (a wave's row group not filled, filled and one over)."""
    for H in (1, 3, 5):
        op = _operands(KINDS[kind], 2, H, W, 32, 64, seed=W * 10 + H, add0=True)
        _assert_layer_exact(KINDS[kind], op, True, f"{kind} H={H} W={W}")


CHANNELS = [(5, 32), (32, 64), (64, 32), (128, 128), (1024, 512), (32, 20)]


@pytest.mark.parametrize("channels", CHANNELS, ids=str)
@pytest.mark.parametrize("kind", list(KINDS))
def test_layer_is_exact_for_every_channel_count(kind, channels):
    cin, cout = channels
    op = _operands(KINDS[kind], 2, 2, 8, cin, cout, seed=cin + cout, add1=True)
    _assert_layer_exact(KINDS[kind], op, True, f"{kind} {cin}->{cout}")


@pytest.mark.parametrize("W", [1, 2, 17])
def test_transposed_conv_is_exact_at_small_widths(W):
    op = _operands(R.KIND_UPCONV, 2, 3, W, 64, 32, seed=W)
    _assert_layer_exact(R.KIND_UPCONV, op, True, f"upconv W_in={W}")


@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("add1", [False, True])
@pytest.mark.parametrize("add0", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_layer_is_exact_with_and_without_each_addend_and_activation(kind, add0, add1, leaky):
    op = _operands(KINDS[kind], 2, 3, 34, 32, 32, seed=4 * add0 + 2 * add1 + leaky, add0=add0, add1=add1)
    _assert_layer_exact(KINDS[kind], op, leaky, f"{kind} add0={add0} add1={add1} leaky={leaky}")


def test_head_argmax_takes_the_lowest_index_on_ties():
    op = _operands(R.KIND_3X3, 2, 5, 34, 32, 20, seed=7)
    # planted ties: classes 3, 7 and 12 share weights, scale and shift (equal logits everywhere), classes 0 and 19 another pair;
    # a block of zero input makes every class with the same shift tie as well
    for group in ((3, 7, 12), (0, 19)):
        for c in group[1:]:
            op["w"][c] = op["w"][group[0]]
            op["scale"][c] = op["scale"][group[0]]
            op["shift"][c] = op["shift"][group[0]]
    op["shift"][[1, 2, 4]] = op["shift"].max() + 1
    op["x"][:, :, :, 10:20] = 0
    got = _device_layer(R.KIND_3X3, op, False, want_argmax=True)
    _, v = R.layer_host(R.KIND_3X3, op["x"], op["w"], op["scale"], op["shift"], False, bf16=True)
    assert torch.equal(got["f32"].cpu(), v)
    want = np.argmax(v.numpy(), axis=1)                  # numpy: the first occurrence of the maximum
    ties = int(((v == v.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
    print(f"{ties} of {want.size} pixels hold a tie for the maximum")
    assert ties > want.size // 4
    assert got["argmax"].dtype == torch.uint8 and np.array_equal(got["argmax"].cpu().numpy(), want.astype(np.uint8))


# ---- 2. zero padding is not wrap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["3x3", "3x3s2", "upconv"])
def test_borders_are_zero_padded_not_wrapped(kind):
    k = KINDS[kind]
    op = _operands(k, 2, 5, 66, 32, 32, seed=11)
    x = torch.zeros_like(op["x"])
    for sl in ((..., 0), (..., -1), (..., 0, slice(None)), (..., -1, slice(None))):
        x[sl] = op["x"][sl]
    x[x == 0] = 1                                        # (no zeros on the border: a wrapped read would always change a sum)
    x[..., 1:-1, 1:-1] = 0
    op["x"] = x
    op["w"][op["w"] == 0] = 1
    _assert_layer_exact(k, op, True, f"{kind} border-only input")
    # the same layer on a wrapped image gives something else: the comparison above can tell the two apart
    _, v = R.layer_host(k, x, op["w"], op["scale"], op["shift"], True, bf16=True)
    if k == R.KIND_UPCONV:
        wrapped = torch.cat([x[..., -1:], x, x[..., :1]], -1)
        _, vw = R.layer_host(k, wrapped, op["w"], op["scale"], op["shift"], True, bf16=True)
        vw = vw[..., 2:-2]
    else:
        wrapped = torch.nn.functional.pad(x, (1, 1, 0, 0), mode="circular")
        wrapped = torch.nn.functional.pad(wrapped, (0, 0, 1, 1))
        acc = torch.nn.functional.conv2d(wrapped, op["w"], stride=(1, 2 if k == R.KIND_3X3_S2 else 1))
        vw = acc * op["scale"].view(1, -1, 1, 1) + op["shift"].view(1, -1, 1, 1)
        vw = torch.where(vw >= 0, vw, vw * torch.tensor(0.1))
    assert vw.shape == v.shape and not torch.equal(vw, v)


# ---- 3. small networks against the reference golden -----------------------------------------------------------------------
def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("layers", [21, 53])
def test_small_network_is_within_twice_the_emulation_of_the_reference(layers):
    state, x, feat_ref, logits_ref = small_case(layers)
    feat_em, logits_em = R.forward_host(state, x, bf16=True)
    bound_f, bound_l = 2 * _rel_l2(feat_em, feat_ref), 2 * _rel_l2(logits_em, logits_ref)
    net = R.RangeNet(state)
    argmax, feat = net.infer(x.cuda())
    logits = net.logits(x.cuda())
    err_f, err_l = _rel_l2(feat.cpu(), feat_ref), _rel_l2(logits.cpu(), logits_ref)
    print(f"DarkNet{layers}: features rel-L2 {err_f:.3e} (bound {bound_f:.3e}), logits {err_l:.3e} (bound {bound_l:.3e}); "
          f"to the emulation {_rel_l2(feat.cpu(), feat_em):.3e} / {_rel_l2(logits.cpu(), logits_em):.3e}")
    assert err_f <= bound_f and err_l <= bound_l
    assert np.array_equal(argmax.cpu().numpy(), np.argmax(logits.cpu().numpy(), axis=1).astype(np.uint8))


# ---- 4. full-size DarkNet53, one scan -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_net():
    g = load_golden()
    return g, R.RangeNet(golden_state(53, g))


def _full_input(g):
    pts, rem = R.synthetic_cloud(FULL_SEED)
    proj, _ = R.project_scan(pts, rem)
    assert zlib.crc32(proj.tobytes()) == int(g["full_input_crc"]), "the seeded scan's projection differs from the golden's input"
    return torch.from_numpy(proj)[None]


def test_full_size_darknet53_matches_the_reference(full_net):
    g, net = full_net
    x = _full_input(g).cuda()
    idx = M.frd_indices()
    argmax, gathered = net.infer(x, gather=idx)
    want = torch.from_numpy(g["full_gathered"])
    err, bound = _rel_l2(gathered.cpu()[0], want), 2 * float(g["full_emul_rel_l2"])
    margin = g["full_margin"].astype(np.float32)
    confident = margin > 4 * float(g["full_emul_logit_err"])
    share = float(confident.mean())
    wrong = int((argmax.cpu().numpy()[0] != g["full_argmax"])[confident].sum())
    print(f"gathered features rel-L2 {err:.3e} (bound {bound:.3e}); {share:.1%} confident pixels, {wrong} of them differ; "
          f"{int((argmax.cpu().numpy()[0] != g['full_argmax']).sum())} of all pixels differ")
    assert share >= 0.9
    assert err <= bound
    assert wrong == 0


# ---- 5. properties --------------------------------------------------------------------------------------------------------
def test_a_scan_does_not_depend_on_its_batch_and_calls_repeat(full_net):
    g, net = full_net
    _, xs, _, _ = small_case(53)
    x3 = torch.cat([xs, xs[:1].flip(-1)], 0).cuda()      # three scans of 8 x 64
    a3, f3 = net.infer(x3)
    l3 = net.logits(x3)
    for i in range(3):
        a1, f1 = net.infer(x3[i:i + 1])
        assert torch.equal(a1[0], a3[i]) and torch.equal(f1[0], f3[i]) and torch.equal(net.logits(x3[i:i + 1])[0], l3[i])
    a3b, f3b = net.infer(x3)
    assert torch.equal(a3, a3b) and torch.equal(f3, f3b)


def test_gather_equals_indexing_the_feature_map(full_net):
    g, net = full_net
    _, xs, _, _ = small_case(53)
    x = xs.cuda()
    total = 32 * x.shape[2] * x.shape[3]
    idx = M.frd_indices(total, 777)
    a_full, f_full = net.infer(x)
    a_g, f_g = net.infer(x, gather=idx)
    assert tuple(f_g.shape) == (2, 777) and torch.equal(a_full, a_g)
    assert torch.equal(f_g, f_full.reshape(2, -1)[:, torch.as_tensor(idx, device=f_full.device)])


# ---- 6. drivers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_dirs(tmp_path_factory):
    """A DarkNet21 model folder and two folders of three seeded clouds each."""
    root = tmp_path_factory.mktemp("rangenet")
    g = load_golden()
    arch = R.synthetic_arch(21)
    R.save_pretrained(str(root / "model"), arch, *R.synthetic_state(arch, int(g["seed"]), R.bn_stats_from_arrays(21, g["bn21_mean"], g["bn21_var"]),
                                                                    head_bias_std=float(g["head_bias_std"])))
    for name, base in (("a", 100), ("b", 200)):
        (root / name).mkdir()
        for i in range(3):
            pts, rem = R.synthetic_cloud(base + i, n=20000)
            np.concatenate([pts, rem[:, None]], 1).astype(np.float32).tofile(str(root / name / f"{i:04d}.bin"))
    return root


@pytest.fixture(scope="module")
def dumped(driver_dirs):
    """`evaluate rangenet` over both cloud folders, one process each: (root, {folder: the JSON line})."""
    root = driver_dirs
    outs = {}
    for name in ("a", "b"):
        args = ["rangenet", "--model", str(root / "model"), "--dump", str(root / name), "--frd-dir", str(root / f"frd_{name}"),
                "--output-dir", str(root / f"seg_{name}")]
        outs[name] = _run_evaluate(1, args, timeout=300)
    return root, outs


def test_evaluate_rangenet_writes_activations_and_segmentations(dumped, tmp_path):
    root, outs = dumped
    assert json.loads(outs["a"]) == {"task": "rangenet", "files": 3, "layers": 21}
    # two ranks write the same files and print the same object
    two = _run_evaluate(2, ["rangenet", "--model", str(root / "model"), "--dump", str(root / "a"), "--frd-dir",
                            str(tmp_path / "frd"), "--output-dir", str(tmp_path / "seg")], timeout=300)
    assert two == outs["a"]
    for i in range(3):
        one_f, two_f = np.load(root / "frd_a" / f"{i}.npy"), np.load(tmp_path / "frd" / f"{i}.npy")
        assert one_f.shape == (1, 32, 64, 1024) and one_f.dtype == np.float32 and np.array_equal(one_f, two_f)
        seg = torch.load(root / "seg_a" / f"{i}.pth", weights_only=True)
        assert tuple(seg.shape) == (64, 1024) and seg.dtype == torch.int64
        assert torch.equal(seg, torch.load(tmp_path / "seg" / f"{i}.pth", weights_only=True))
    acts = M.load_activations(str(root / "frd_a"), M.frd_indices(), device="cpu")
    assert tuple(acts.shape) == (3, 4096) and acts.dtype == torch.float32 and bool(acts.std() > 0)


def test_evaluate_frd_from_clouds_equals_frd_from_the_dumps(dumped):
    """byte for byte, for one and two ranks"""
    root, _ = dumped
    dumps = _run_evaluate(1, ["frd", str(root / "frd_a"), str(root / "frd_b")], timeout=300)
    direct = _run_evaluate(1, ["frd", "--rangenet", str(root / "model"), str(root / "a"), str(root / "b")], timeout=300)
    direct2 = _run_evaluate(2, ["frd", "--rangenet", str(root / "model"), str(root / "a"), str(root / "b")], timeout=300)
    assert direct == dumps and direct2 == dumps
    res = json.loads(direct)
    assert res["n1"] == 3 and res["n2"] == 3 and res["dims"] == 4096 and res["frd"] > 0


def test_evaluate_segmentation(dumped):
    root, _ = dumped
    # a folder against itself: perfect agreement; against the other folder: a proper fraction, the same for two ranks
    same = json.loads(_run_evaluate(1, ["segmentation", str(root / "seg_a"), str(root / "seg_a")], timeout=300))
    assert same == {"task": "segmentation", "iou": 1.0, "accuracy": 1.0, "n": 3}
    other = _run_evaluate(1, ["segmentation", str(root / "seg_a"), str(root / "seg_b")], timeout=300)
    assert _run_evaluate(2, ["segmentation", str(root / "seg_a"), str(root / "seg_b")], timeout=300) == other
    res = json.loads(other)
    assert 0.0 <= res["iou"] <= res["accuracy"] < 1.0
    segs = [torch.load(root / f"seg_{n}" / f"{i}.pth", weights_only=True) for n in "ab" for i in range(3)]
    want = R.segmentation_scores(torch.stack(segs[:3]), torch.stack(segs[3:]))
    assert res["iou"] == want["iou"] and res["accuracy"] == want["accuracy"]
