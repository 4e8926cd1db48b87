"""GPU: the order-fixed BEV splat (rldm_lidar_to_voxel_ordered; to_voxel / to_voxel_train with ordered=True) and the BEV terms of the VAE
trainers under deterministic=True, bev_ordered=True.

  bit-exact     raw (d and S) of to_voxel_train(ordered=True) against range_image.to_voxel_ordered_host on the device's own points, bit
                patterns compared: tests/bev_util.py's input on both small grids and all modes, and the crowded input of
                tests/test_bev_ordered_host.py (20 sort chunks an image, cells of ~1900 votes fed by every chunk, a ragged last round) on
                the 1x4x4, 1x5x7 and -- a second digit pass -- 1x64x64 grids.  tests/test_bev_ordered_host.py shows on the CPU that
                these inputs give other bits when a cell is summed in another order.
  finalise      voxel is the existing out-of-place finalise of that raw; the inference call returns the training call's bits
  independence  of the batch size, the batch position and the run
  non-finite    the rule of test_hip_splat_nonfinite_pixels_and_batch_slots, here bit for bit
  bounds        to_voxel(ordered=True) inside splat_bounds of the fp64 reference, the gate to_voxel passes
  backward      to_voxel_backward on the ordered accumulators, under test_backward_within_the_rounding_bound's bound
  trainers      two deterministic trainers with bev_ordered=True end with the same bits; the step against autograd and Adam under
                tests/test_bev_training_gpu.py's own gates; the switch alone changes nothing; refusals; the command line twice
"""
import filecmp
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd import discriminator as D
from tests import bev_util as BU
from tests import test_bev_ordered_host as OH
from tests.test_lidar_exact import bits

pytestmark = pytest.mark.gpu
F = np.float32
U = BU.U
GRID_CASES = pytest.mark.parametrize("grid,pc_range", BU.SPLAT_GRIDS, ids=BU.SPLAT_IDS)
MODE_CASES = pytest.mark.parametrize("mode", BU.MODES)
CROWD_CASES = pytest.mark.parametrize("grid,pc_range,width", [OH.CROWD_GRID + (OH.CROWD_W,), OH.ODD_GRID + (OH.CROWD_W,),
                                                              OH.WIDE_GRID + (OH.WIDE_W,)], ids=["1x4x4", "1x5x7", "1x64x64"])


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def ordered_raw(t, img):
    """-> (voxel, raw) of to_voxel_train(ordered=True) as numpy, the device's points."""
    x = dev(img)
    vox, (kept, raw) = t.to_voxel_train(x, ordered=True)
    assert torch.equal(kept, x) and vox.shape == raw.shape and vox.dtype == raw.dtype == torch.float32
    return vox.cpu().numpy(), raw.cpu().numpy(), t.to_pc_torch(x).cpu().numpy()


def check_against_host(t, img):
    """raw against the host statement bit for bit; voxel against the finalise step of that raw; the inference call's bits."""
    gz = int(t.grid_sizes[0])
    vox, raw, pts = ordered_raw(t, img)
    _, d, S = t.to_voxel_ordered_host(img, points=pts)
    assert np.array_equal(bits(raw[:, :gz]), bits(d)), int((bits(raw[:, :gz]) != bits(d)).sum())
    assert np.array_equal(bits(raw[:, gz:]), bits(S)), int((bits(raw[:, gz:]) != bits(S)).sum())
    assert np.array_equal(bits(t.to_voxel(dev(img), ordered=True).cpu().numpy()), bits(vox))
    # bev_finalize_train_kernel on that raw: an empty cell keeps raw's bits; the density plane is d itself or logf(d + 1) (the project's
    # 2e-5 for logf, as test_hip_splat_cell_by_cell); the feature plane is one fp32 division S / max(d, float32(1e-4)), allowed one
    # ulp beyond the correctly rounded quotient (2 u |q|)
    occ = d != 0
    assert np.array_equal(bits(vox[:, :gz])[~occ], bits(d)[~occ]) and np.array_equal(bits(vox[:, gz:])[~occ], bits(S)[~occ])
    if t.normalize_volume_densities:
        assert (np.abs(vox[:, :gz].astype(np.float64) - np.log1p(d.astype(np.float64))) <= 2e-5).all()
    else:
        assert np.array_equal(bits(vox[:, :gz]), bits(d))
    q = S.astype(np.float64) / np.maximum(d, F(1e-4)).astype(np.float64)
    assert (np.abs(vox[:, gz:].astype(np.float64) - q)[occ] <= 2 * U * np.abs(q)[occ] + 2.0 ** -149).all()
    return vox, raw


# ---- bit-exact ----------------------------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_ordered_splat_bit_exact_on_bev_input(grid, pc_range, mode):
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    for normalize in (False, True):
        check_against_host(BU.bev_sensor(grid, pc_range, mode, normalize), img)


@CROWD_CASES
@MODE_CASES
def test_ordered_splat_bit_exact_crowded_and_multi_chunk(grid, pc_range, width, mode):
    """The crowded input (tests/test_bev_ordered_host.py: crowded_input and the constants above it).  csrc/lidar.hip sorts in chunks of
    ORD_CHUNK = 1024 vote positions, one wave each, four to a workgroup, in rounds of 64.  At W = 509 an image has 8 * 509 * 5 = 20 360
    positions: 20 chunks in 5 workgroups, the last chunk 904 long and its last round 8 lanes wide; the four centre cells of the 1x4x4 grid
    hold ~1900 votes each, from every chunk (asserted on the CPU), and are summed by the wave in ~30 loads of 64 with a ragged last one.
    The 1x5x7 grid has 35 cells (no power of two); the 1x64x64 grid at W = 64 needs 13 key bits, a second digit pass."""
    vox, _ = check_against_host(OH.crowd_sensor(grid, pc_range, mode, width, normalize=False), np.array(OH.crowded_input(mode, width)))
    assert np.isfinite(vox).all()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------
@MODE_CASES
def test_ordered_splat_does_not_depend_on_batch_position_or_run(mode):
    grid, pc_range = OH.CROWD_GRID
    t = OH.crowd_sensor(grid, pc_range, mode, OH.CROWD_W)
    img = np.array(OH.crowded_input(mode))
    vox, raw, _ = ordered_raw(t, img)
    vox2, raw2, _ = ordered_raw(t, img)
    assert np.array_equal(bits(raw), bits(raw2)) and np.array_equal(bits(vox), bits(vox2))                   # run to run
    _, alone, _ = ordered_raw(t, img[:1])
    assert np.array_equal(bits(alone[0]), bits(raw[0]))                                                      # B = 1 against B = 3
    _, moved, _ = ordered_raw(t, img[[1, 2, 0]])
    assert np.array_equal(bits(moved[2]), bits(raw[0])) and np.array_equal(bits(moved[0]), bits(raw[1]))     # batch position 2


# ---- non-finite pixels ------------------------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_ordered_splat_nonfinite_pixels_and_batch_slots(grid, pc_range, mode):
    """A NaN / +inf / -inf pixel casts no vote unless it decodes to a finite point inside the volume (the rule of
    test_hip_splat_nonfinite_pixels_and_batch_slots): where it casts none, image 0's accumulators are, bit for bit, those of the image
    with that pixel moved far outside -- the other votes keep their order --; always the host statement's on the device's points, finite,
    and batch slot 1 untouched."""
    t = BU.bev_sensor(grid, pc_range, mode, normalize=False)
    o = BU.oracle_of(t)
    img = BU.splat_input(mode)
    inside = o.votes(o.to_pc(img))[2][0].sum(1)
    n0 = int(np.argmax(inside))
    assert inside[n0] >= 4
    w0, h0 = divmod(n0, 5)
    moved = img.copy()
    moved[0, 0, w0, h0] = BU.encode(3000.0, mode)
    _, raw_moved = check_against_host(t, moved)
    _, raw_clean = check_against_host(t, img)
    assert not np.array_equal(bits(raw_moved[0]), bits(raw_clean[0]))
    dropped = 0
    for bad in (np.nan, np.inf, -np.inf):
        image = img.copy()
        image[0, 0, w0, h0] = bad
        vox, raw = check_against_host(t, image)
        assert np.isfinite(vox).all() and np.isfinite(raw).all()
        assert np.array_equal(bits(raw[1]), bits(raw_clean[1]))
        pc = t.to_pc_torch(dev(image)).cpu().numpy()
        if not np.isfinite(pc[0, n0, :3]).all() or not o.votes(np.where(np.isfinite(pc), pc, F(1e6)))[2][0, n0].any():
            assert np.array_equal(bits(raw[0]), bits(raw_moved[0]))
            dropped += 1
        else:
            assert mode == "inverse" and bad == np.inf
    assert dropped >= 2


# ---- ordered against the fp64 reference -------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_ordered_splat_within_splat_bounds(grid, pc_range, mode):
    """test_hip_splat_cell_by_cell's gate (its docstring derives the bounds: they cover a k-term fp32 sum in any order)."""
    img = BU.splat_input(mode)
    x = dev(img)
    gz = grid[0]
    for normalize in (False, True):
        t = BU.bev_sensor(grid, pc_range, mode, normalize)
        o = BU.oracle_of(t)
        pc = t.to_pc_torch(x).cpu().numpy()
        got = t.to_voxel(x, ordered=True).cpu().numpy().astype(np.float64)
        want = o.to_voxel(img, pc=pc).astype(np.float64)
        ref = BU.splat_reference(o, pc)
        _, bound_d, bound_f = BU.splat_bounds(ref)
        occ = ref["k"] > 0
        assert np.isfinite(got).all() and (got[:, gz:][~occ] == 0).all() and (got[:, :gz][~occ] == 0).all()
        if not normalize:
            assert np.array_equal(got[:, :gz] != 0, occ)
        assert (np.abs(got[:, :gz] - want[:, :gz]) <= bound_d + (2e-5 if normalize else 0.0)).all()
        assert (np.abs(got[:, gz:] - want[:, gz:]) <= bound_f).all()


# ---- backward -----------------------------------------------------------------------------------------------------------------------------------
def test_backward_reads_the_ordered_accumulators():
    """to_voxel_backward is unchanged and reads `raw` whichever forward wrote it: one grid, one mode, against to_voxel_backward_host on
    the ordered accumulators under the bound test_backward_within_the_rounding_bound derives (CHAIN u sum |terms|)."""
    from tests.test_bev_training_gpu import CHAIN
    (grid, pc_range), mode = BU.SPLAT_GRIDS[0], "linear"
    t = BU.bev_sensor(grid, pc_range, mode)
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    x = dev(img)
    gz = grid[0]
    G = BU.upstream((BU.SPLAT_B, 2 * gz, grid[1], grid[2]))
    _, saved = t.to_voxel_train(x, ordered=True)
    got = t.to_voxel_backward(saved, dev(G))
    assert torch.equal(got, t.to_voxel_backward(saved, dev(G)))
    got = got.cpu().double()
    raw = saved[1].cpu()
    want, terms = t.to_voxel_backward_host(torch.from_numpy(img), raw[:, :gz], raw[:, gz:], torch.from_numpy(G),
                                           points=t.to_pc_torch(x).cpu(), return_terms=True, tables="library")
    err, bound = (got - want).abs(), CHAIN * U * terms
    assert torch.isfinite(got).all() and float(want.abs().max()) > 0.1
    assert (err <= bound).all(), float((err[terms > 0] / bound[terms > 0]).max())


# ---- trainers ---------------------------------------------------------------------------------------------------------------------------------
def _bits(tr):
    return [t.cpu().clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


def _batches(o, n=3, seed=5):
    """Images near the case's target (reconstructions and targets inside the 32 m volume) and latents near its z."""
    g = torch.Generator().manual_seed(seed)
    return [((o["target"] + 0.01 * torch.randn(o["target"].shape, generator=g)).contiguous(),
             (o["z"] + 0.1 * torch.randn(o["z"].shape, generator=g)).contiguous()) for _ in range(n)]


def _run(which, o, batches, disc_cfg, **kw):
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    disc = D.PatchDiscriminator(disc_cfg, seed=3, lr=1e-3, deterministic=True)
    if which == "all":
        tr = VAETrainer(o["cfg"], o["sd"], lr=1e-3, deterministic=True, discriminator=disc, disc_start=1, **kw)
        losses = [float(tr.train_step(x.cuda(), noise=torch.zeros_like(z).cuda())) for x, z in batches]
    else:
        tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=1e-3, deterministic=True, discriminator=disc, disc_start=1, **kw)
        losses = [float(tr.train_step(z.cuda(), x.cuda())) for x, z in batches]
    assert tr.last_disc is not None and tr.global_step == len(batches)
    state = _bits(tr) + _bits(disc) + [disc.buffers[k].cpu().clone() for k in sorted(disc.buffers)]
    return tr, losses, state


@pytest.mark.parametrize("variant", ["bev_rec", "disc_bev", "both"])
@pytest.mark.parametrize("which", ["decoder", "all"])
def test_bev_terms_train_bit_reproducibly(which, variant):
    """deterministic=True, bev_ordered=True, a deterministic PatchGAN, disc_start = 1: two trainers on the same three batches end with
    the same parameter, optimizer and discriminator bits and return the same losses."""
    from tests.test_bev_training_gpu import DCFG, train_case
    o = train_case()
    kw = dict(bev_rec_weight=1.0) if variant == "bev_rec" else dict(disc_bev=True) if variant == "disc_bev" else dict(bev_rec_weight=1.0, disc_bev=True)
    disc_cfg = DCFG if kw.get("disc_bev") else D.DiscriminatorConfig(2, 16, 1)           # 32 x 32 volumes / 32 x 8 images
    batches = _batches(o)
    runs = []
    for _ in range(2):
        tr, losses, state = _run(which, o, batches, disc_cfg, bev=BU.train_sensor(), bev_ordered=True, **kw)
        assert tr.bev_ordered and all(np.isfinite(losses))
        if "bev_rec_weight" in kw:
            assert float(tr.last_bev_rec) > 0                                              # the term is alive: volumes are occupied
        runs.append((losses, state))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize("which", ["decoder", "all"])
def test_bev_ordered_alone_leaves_the_step_bit_identical(which):
    """bev_ordered=True without a BEV term is accepted and never read: the same bits as a trainer without it."""
    from tests.test_bev_training_gpu import train_case
    o = train_case()
    batches = _batches(o)
    cfg = D.DiscriminatorConfig(2, 16, 1)
    _, l0, s0 = _run(which, o, batches, cfg)
    tr, l1, s1 = _run(which, o, batches, cfg, bev=BU.train_sensor(), bev_ordered=True)
    assert tr.last_bev_rec is None
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(s0, s1))


@pytest.mark.parametrize("variant", ["bev_rec", "disc_bev", "both"])
def test_train_step_with_ordered_bev_terms_matches_autograd_and_adam(variant, capsys):
    """test_train_step_with_bev_terms_matches_autograd_and_adam (tests/test_bev_training_gpu.py) with bev_ordered=True: its case, its
    host_step, its gates (STEP_GATES of tests/test_discriminator_gpu.py, and 4e-5 per occupied cell for last_bev_rec), unchanged."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    from tests.test_bev_training_gpu import BEV_W, VARIANTS, _adam_figures, host_step, train_case
    from tests.test_discriminator_gpu import STEP_GATES, _param_errors
    o = train_case()
    kw = dict(VARIANTS[variant])
    disc = D.PatchDiscriminator(state=o["dstate"], lr=o["lr"]) if kw.get("disc_bev") else None
    tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=o["lr"], discriminator=disc, disc_start=0, bev=BU.train_sensor(), bev_ordered=True, **kw)
    snap = {}
    step = tr.optimizer_step

    def keep_then_step():
        snap.update({n: tr.g[n].cpu().clone() for n in tr.names})
        return step()
    tr.optimizer_step = keep_then_step
    loss = tr.train_step(o["z"].cuda(), o["target"].cuda())
    torch.cuda.synchronize()
    ref = host_step(o, dict(kw, **({"dstate": o["dstate"]} if disc is not None else {})), tr.sample_nchw().cpu())
    assert ref["occupied"] >= 100 and ref.get("bias_conditioning", 1.0) >= 0.5
    fig = {}
    w, n, a = _param_errors(snap, ref["grads"], tr.names)
    fig.update(grad_worst=w, grad_all=a)
    init = {k: torch.from_numpy(o["sd"][k]).float() for k in o["keys"]}
    if "bev_rec_weight" in kw:
        got = float(tr.last_bev_rec)
        assert abs(got - ref["bev_rec"]) <= 4e-5 * ref["cells"], (got, ref["bev_rec"])
        assert ref["bev_rec"] > 1.0 and abs(float(loss) - (ref["l1"] + BEV_W / o["B"] * ref["bev_rec"])) <= 1e-5 * float(loss)
    if disc is not None:
        fig["g_loss"] = abs(float(tr.last_g_loss) - ref["g_loss"]) / abs(ref["g_loss"])
        fig["d_weight"] = abs(float(tr.last_d_weight) - ref["d_weight"]) / ref["d_weight"]
        fig["adam_beyond_half_step"], fig["adam_rel"] = _adam_figures(disc.state_dict(), ref["dparams"], o["dstate"], disc.names, o["lr"])
    else:
        fig["adam_beyond_half_step"], fig["adam_rel"] = _adam_figures(tr.state_dict(), ref["params"], init, tr.names, o["lr"])
    with capsys.disabled():
        print(f"\nordered {variant}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()) + f"; worst gradient {n}")
    bad = {k: (v, STEP_GATES[k]) for k, v in fig.items() if not v <= STEP_GATES[k]}
    assert not bad, bad


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_switch_and_oversize_shapes_are_refused():
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    from tests.test_bev_training_gpu import DCFG, train_case
    o = train_case()
    cfg, sd, bev = o["cfg"], o["sd"], BU.train_sensor()
    patch = D.PatchDiscriminator(DCFG, seed=1, deterministic=True)
    for cls in (VAEDecoderTrainer, VAETrainer):
        with pytest.raises(NotImplementedError, match="atomics.*bev_ordered"):
            cls(cfg, sd, bev=bev, bev_rec_weight=1.0, deterministic=True)
        with pytest.raises(NotImplementedError, match="atomics.*bev_ordered"):
            cls(cfg, sd, bev=bev, discriminator=patch, disc_bev=True, deterministic=True, bev_ordered=False)
        cls(cfg, sd, bev=bev, discriminator=patch, disc_bev=True, bev_rec_weight=1.0, deterministic=True, bev_ordered=True)
        cls(cfg, sd, bev=bev, bev_rec_weight=1.0, bev_ordered=True)                        # ordered splat, unordered step: allowed
        cls(cfg, sd, bev_ordered=True, deterministic=True)                                 # no BEV term: accepted, never read
        with pytest.raises(ValueError, match="bev="):
            cls(cfg, sd, bev_rec_weight=1.0, bev_ordered=True)
    # the C ABI refuses before it touches memory: 8 * B * W * beams >= 2^31 votes, and a grid of 2^31 cells
    t = BU.bev_sensor(*BU.SPLAT_GRIDS[1], "linear")
    x = torch.zeros(1, 2, 37, 5, device="cuda")
    buf = torch.zeros(64, device="cuda")
    call = _lib.lib().rldm_lidar_to_voxel_ordered
    st = _lib.stream_ptr(x.device)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        _lib.check(call(t._handle(), x.data_ptr(), 1 << 16, 2, 1 << 10, buf.data_ptr(), buf.data_ptr(), st), "rldm_lidar_to_voxel_ordered")
    _lib.check(call(t._handle(), x.data_ptr(), 1, 2, 37, buf.data_ptr(), buf.data_ptr() + 128, st), "rldm_lidar_to_voxel_ordered")
    with pytest.raises(RuntimeError, match="remission"):
        _lib.check(call(t._handle(), x.data_ptr(), 1, 1, 37, buf.data_ptr(), buf.data_ptr(), st), "rldm_lidar_to_voxel_ordered")
    with pytest.raises(RuntimeError, match="null"):
        _lib.check(call(t._handle(), x.data_ptr(), 1, 2, 37, None, buf.data_ptr(), st), "rldm_lidar_to_voxel_ordered")
    big = OH.FiveSteep(width=37, grid_sizes=[8, 1 << 14, 1 << 14], pc_range=[-4., -4., -3., 4., 4., 1.])
    with pytest.raises(RuntimeError, match="fewer than 2\\^31 cells"):
        _lib.check(call(big._handle(), x.data_ptr(), 1, 2, 37, buf.data_ptr(), buf.data_ptr(), st), "rldm_lidar_to_voxel_ordered")
    torch.cuda.synchronize()


# ---- command line -------------------------------------------------------------------------------------------------------------------------------
def test_command_line_is_byte_reproducible_with_bev_ordered(tmp_path, capsys):
    """train_vae --deterministic --bev-ordered --disc-bev --bev-rec-weight 1 --discriminator patchgan, twice, in process, two steps at
    the small shape of test_command_line_runs_the_bev_terms: OUT/vae/ and OUT/discriminator.pt are byte-identical.  Without
    --bev-ordered the old ValueError stays."""
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae_training import save_vae_dir
    from tests.test_vae_training_gpu import TALL
    sd = synth_state_dict(vae_param_shapes(TALL), prefix="vt.")
    src = tmp_path / "src"
    save_vae_dir(str(src), TALL, sd)
    base = ["--weights", str(src), "--steps", "2", "--batch-size", "2", "--lr", "1e-3", "--log-every", "1", "--seed", "4", "--deterministic",
            "--discriminator", "patchgan", "--disc-start", "1", "--disc-bev", "--bev-rec-weight", "1", "--bev-grid", "1", "32", "32"]
    outs, logs = [tmp_path / "a", tmp_path / "b"], []
    for out in outs:
        CLI.main(base + ["--out", str(out), "--bev-ordered"])
        logs.append([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")])
    assert len(logs[0]) == 2 and logs[0] == logs[1] and '"bev_rec"' in logs[0][0] and '"g_loss"' in logs[0][1]
    files = sorted(os.path.relpath(os.path.join(r, f), outs[0]) for r, _, fs in os.walk(outs[0]) for f in fs)
    assert "discriminator.pt" in files and any(f.startswith("vae" + os.sep) for f in files)
    match, mismatch, errors = filecmp.cmpfiles(outs[0], outs[1], files, shallow=False)
    assert sorted(match) == files and not mismatch and not errors, (mismatch, errors)
    with pytest.raises(ValueError, match="--deterministic"):
        CLI.main(base + ["--out", str(tmp_path / "c")])
