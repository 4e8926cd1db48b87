"""GPU: the differentiable to_voxel (range_image.to_voxel_train / to_voxel_backward, csrc/lidar.hip) and the BEV terms of the VAE
trainers (vae_training.py: bev_rec_weight, disc_bev).

  forward    to_voxel_train's output planes within the per-cell bounds test_hip_splat_cell_by_cell derives, on its shapes; the raw
             accumulators within the density bound (and the numerator's E_n); to_voxel on the same input within the same bounds
  backward   against to_voxel_backward_host on the DEVICE'S OWN accumulators, points and image, so the order of the forward's atomics
             drops out: per output element c 2^-24 sum |terms| (c derived in test_backward_within_the_rounding_bound)
  end to end device forward + backward against fp64 autograd of to_voxel_host, relative L2, gated at 4 x the distance between fp32 and
             fp64 autograd of that same statement
  trainer    one train_step with bev_rec_weight alone, disc_bev alone, and both, against torch autograd / torch Adam; defaults,
             refusals, state round trip, command line

The inputs are tests/bev_util.py's; tests/test_bev_training_host.py shows on the CPU that they reach every class of pixel."""
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import discriminator as D
from tests import bev_util as BU

pytestmark = pytest.mark.gpu
GRID_CASES = pytest.mark.parametrize("grid,pc_range", BU.SPLAT_GRIDS, ids=BU.SPLAT_IDS)
MODE_CASES = pytest.mark.parametrize("mode", BU.MODES)
U = BU.U


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_forward_keeps_the_accumulators_and_to_voxels_bounds(grid, pc_range, mode, capsys):
    """test_hip_splat_cell_by_cell's comparison (its docstring derives the bounds) for to_voxel_train's output planes, for the raw planes
    -- d within bound_d, S within E_n + u |n|, both against the fp64 accumulation of the device's own fp32 votes -- and for to_voxel."""
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    x = dev(img)
    gz = grid[0]
    worst = {}
    for normalize in (False, True):
        t = BU.bev_sensor(grid, pc_range, mode, normalize)
        o = BU.oracle_of(t)
        pc = t.to_pc_torch(x).cpu().numpy()
        vox, (kept, raw) = t.to_voxel_train(x)
        assert torch.equal(kept, x) and vox.shape == raw.shape == (BU.SPLAT_B, 2 * gz, grid[1], grid[2])
        plain = t.to_voxel(x).cpu().numpy().astype(np.float64)
        vox, raw = vox.cpu().numpy().astype(np.float64), raw.cpu().numpy().astype(np.float64)
        want = o.to_voxel(img, pc=pc).astype(np.float64)
        ref = BU.splat_reference(o, pc)
        _, bound_d, bound_f = BU.splat_bounds(ref)
        occ = ref["k"] > 0
        km1 = np.maximum(ref["k"] - 1, 0)
        e_n = U * ref["swf_abs"] + km1 * U / (1 - km1 * U) * (1 + U) * ref["swf_abs"]
        assert np.array_equal(raw[:, :gz] != 0, occ) and (raw[:, gz:][~occ] == 0).all()
        assert (np.abs(raw[:, :gz] - ref["sw"]) <= bound_d).all()
        assert (np.abs(raw[:, gz:] - ref["swf"]) <= e_n + U * np.abs(ref["swf"])).all()
        if not normalize:
            assert np.array_equal(vox[:, :gz], raw[:, :gz])                               # the density plane IS the accumulator
        for name, got in (("train", vox), ("to_voxel", plain)):
            assert np.isfinite(got).all() and (got[:, gz:][~occ] == 0).all() and (got[:, :gz][~occ] == 0).all()
            err_d, err_f = np.abs(got[:, :gz] - want[:, :gz]), np.abs(got[:, gz:] - want[:, gz:])
            assert (err_d <= bound_d + (2e-5 if normalize else 0.0)).all(), name
            assert (err_f <= bound_f).all(), name
            worst[name] = max(worst.get(name, 0.0), float((err_f[occ] / bound_f[occ]).max()),
                              float((err_d[occ] / (bound_d[occ] + (2e-5 if normalize else 0.0))).max()))
    with capsys.disabled():
        print(f"\nto_voxel_train {grid} {mode}: largest error / bound  " + "  ".join(f"{n} {v:.3f}" for n, v in sorted(worst.items())))


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
CHAIN = 32


@GRID_CASES
@MODE_CASES
@pytest.mark.parametrize("normalize", (True, False), ids=("log-density", "density"))
def test_backward_within_the_rounding_bound(grid, pc_range, mode, normalize, capsys):
    """to_voxel_backward against to_voxel_backward_host(image, the device's d and S, dvoxel, points = the device's to_pc_torch output,
    tables = the library's): cells, remainders and in-grid tests are then the same fp32 numbers on both sides (the host restates the
    forward's expressions one rounding at a time), the host gathers in fp64, and what differs is the rounding of the device's fp32
    chain.  With u = 2^-24 every fp32 operation errs by at most u relative to its result, and an element of the output is a sum of
    products, so |device - host| <= c u sum |terms| with c the longest chain of roundings a term passes (terms: every product the
    gather adds, with |a1| + |a2| + |f e| in place of |q|; to_voxel_backward_host returns their sum).  The range channel's chain:

        a2 = gF S / (d d)            3     (a1 = gD / (d + 1): 2; e: 1; f e: 2)
        a = a1 - a2                  1
        q = a + f e                  1
        wy wz (of exact remainders)  1
        q (wy wz)                    1
        dpx: 8 terms added           7
        kx = 0.5 (gx - 1) / hx       1
        dpx kx, ci, cos_azi          3
        (gx + gy) - gz               2
        drdv                         linear 0; inverse v v, -1 / .: 2; log: the constant 6 ln 2, v 6 (which moves 2^(6 v) by at
                                     most 6 |v| ln 2 u <= 5 u for |v| <= 1.2), exp2f (2 ulp = 4 u), the product: 11
        times drdv                   1
                                     -- 21 + 11 = 32 at the most; the remission channel's (w: 2, e: 1, w e: 1, 7 additions) is 11.

    c = CHAIN = 32 for every element; second-order terms (1 + u)^32 - 1 - 32 u are 1e-13 relative.  Pixels the forward dropped are
    exactly 0 in both channels, pixels whose range was replaced exactly 0 in the range channel.  Nothing is tuned; the largest
    error / bound is printed."""
    t = BU.bev_sensor(grid, pc_range, mode, normalize)
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    x = dev(img)
    gz = grid[0]
    G = BU.upstream((BU.SPLAT_B, 2 * gz, grid[1], grid[2]))
    _, saved = t.to_voxel_train(x)
    got = t.to_voxel_backward(saved, dev(G))
    assert got.shape == (BU.SPLAT_B, 2, BU.SPLAT_W, 5) and got.dtype == torch.float32
    again = t.to_voxel_backward(saved, dev(G))
    assert torch.equal(got, again)                                                        # a gather in a fixed order: no atomics
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    pts = t.to_pc_torch(x).cpu()
    raw = saved[1].cpu()
    want, terms = t.to_voxel_backward_host(torch.from_numpy(img), raw[:, :gz], raw[:, gz:], torch.from_numpy(G), points=pts,
                                           return_terms=True, tables="library")
    c = BU.pixel_classes(t, img, points=pts)
    dropped, replaced = torch.from_numpy(c["dropped"]), torch.from_numpy(c["replaced"])
    assert dropped.sum() >= 40 and (got[:, 0][dropped] == 0).all() and (got[:, 1][dropped] == 0).all()
    assert (got[:, 0][replaced] == 0).all() and (want[:, 0][replaced] == 0).all() and (want[:, 0][dropped] == 0).all()
    if mode != "inverse":
        assert replaced.sum() >= 20
    live = ~dropped
    assert float(got[:, 0][live].abs().min()) >= 0 and (got[:, 0][live & ~replaced] != 0).float().mean() > 0.9
    err, bound = (got - want).abs(), CHAIN * U * terms
    ratio = float((err[terms > 0] / bound[terms > 0]).max())
    with capsys.disabled():
        print(f"\nto_voxel_backward {grid} {mode} {'log-density' if normalize else 'density'}: largest error / bound {ratio:.3f}, "
              f"largest |gradient| {float(want.abs().max()):.3g}")
    assert (err <= bound).all(), ratio


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_gradient_end_to_end_against_fp64_autograd(grid, pc_range, mode, capsys):
    """Device forward + backward against fp64 autograd of to_voxel_host (the library's tables), relative L2, on the dense image of the
    input (image 0: the planted pixels of image 1 sit ON a kink of the trilinear weights, where fp32 and fp64 take different sides and
    no gradient is defined).  The gate is 4 x the distance between fp32 and fp64 autograd of that same statement, computed here: device
    atomics and torch's index_add_ are both fp32 sums of the same votes in different orders, so their distances to fp64 are of one size
    but independent.
    Measured on an MI355X (device distance / gate): 3x7x5 linear 2.18e-05 / 8.58e-05, log 1.85e-05 / 7.39e-05, inverse 2.21e-05 /
    8.70e-05; 1x4x4 linear 3.40e-07 / 1.41e-06, log 3.87e-07 / 1.51e-06, inverse 2.83e-07 / 1.17e-06."""
    t = BU.bev_sensor(grid, pc_range, mode)
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])[:1]
    G = BU.upstream((1, 2 * grid[0], grid[1], grid[2]))
    grads = []
    for dt in (torch.float32, torch.float64):
        xh = torch.from_numpy(img).to(dt).requires_grad_()
        vox = t.to_voxel_host(xh, tables="library")
        grads.append(torch.autograd.grad((vox * torch.from_numpy(G).to(dt)).sum(), xh)[0].double().numpy())
    gate = 4 * BU.rel_l2(grads[0], grads[1])
    vox_d, saved = t.to_voxel_train(dev(img))
    got = t.to_voxel_backward(saved, dev(G)).cpu().numpy()
    dist = BU.rel_l2(got, grads[1])
    with capsys.disabled():
        print(f"\nto_voxel gradient {grid} {mode}: device against fp64 autograd {dist:.3g}, gate {gate:.3g}")
    assert np.abs(grads[1]).max() > 0.1 and gate < 1e-3
    assert dist <= gate


# ---- trainers ---------------------------------------------------------------------------------------------------------------------------
# tests/test_vae_training_gpu.py's SMALL (32 x 8 images), B = 2; the 8-beam sensor and the [1, 32, 32] grid of tests/bev_util.py; the
# PatchGAN with ndf = 16 and the reference's three layers: 32 x 32 -> 16 -> 8 -> 4 -> 3 -> 2 x 2 logits.
WC = (40.0, 10.0)
DCFG = D.DiscriminatorConfig(2, 16, 3)
BEV_W = 0.5
_CASE = {}
VARIANTS = {"bev_rec": dict(bev_rec_weight=BEV_W), "disc_bev": dict(disc_bev=True), "both": dict(bev_rec_weight=BEV_W, disc_bev=True)}


def train_case():
    """Once: SMALL's weights with conv_out rescaled so that the reconstruction is a plausible range image (range values around -0.3:
    8 m, inside the 32 m volume), a latent batch, a target with the L1 sign margin of tests/test_vae_training_gpu.py, the
    discriminator's state.  The target lies ABOVE the reconstruction in three pixels of four, not in two: decoder.conv_out.bias has
    two elements, each the sum of d loss / d pred over all pixels, and with balanced signs that sum is what is left when the L1's
    part and d_weight times the generator term's part cancel (measured at balanced signs: -125 + 170 = 45) -- a figure relative to
    it then states the cancellation, not the kernels.  host_step returns the conditioning of that sum and the test asserts it."""
    if not _CASE:
        from oracle import vae as o_vae
        from rangeldm_amd.params import vae_param_shapes
        from rangeldm_amd.synth import synth_state_dict
        from tests.test_vae_training_gpu import SMALL
        cfg, B, lr = SMALL, 2, 1e-3
        sd = {k: np.array(v) for k, v in synth_state_dict(vae_param_shapes(cfg), prefix="vt.").items()}
        g = torch.Generator().manual_seed(11)
        f = cfg.downscale
        z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        keys = [k for k in sd if k.startswith("decoder.")]
        raw = o_vae.vae_decode.__wrapped__({k: torch.from_numpy(sd[k]).float() for k in keys}, cfg, z)
        scale = 0.1 / raw.std((0, 2, 3))                                                   # per channel: std 0.1 ...
        sd["decoder.conv_out.weight"] = (sd["decoder.conv_out.weight"] * scale.numpy()[:, None, None, None]).astype(np.float32)
        shift = torch.tensor([-0.3, 0.5]) - raw.mean((0, 2, 3)) * scale                     # ... around -0.3 (8 m) and 0.5
        sd["decoder.conv_out.bias"] = (sd["decoder.conv_out.bias"] * scale.numpy() + shift.numpy()).astype(np.float32)
        pred = o_vae.vae_decode.__wrapped__({k: torch.from_numpy(sd[k]).float() for k in keys}, cfg, z)
        s = (torch.rand(pred.shape, generator=g) < 0.75).float() * 2 - 1
        target = (pred + s * (0.05 + 0.05 * torch.rand(pred.shape, generator=g))).contiguous()
        _CASE.update(cfg=cfg, B=B, lr=lr, sd=sd, z=z, keys=keys, target=target, dstate=D.init_state(DCFG, 3))
    return _CASE


def host_step(o, kw, pred_dev):
    """torch autograd of L1 + bev term + d_weight g_loss (d_weight detached) through the oracle decoder, to_voxel_host and
    discriminator.forward_host, EVALUATED AT THE DEVICE'S RECONSTRUCTION: pred = oracle(pred) + (pred_dev - oracle(pred)).detach().  The
    BEV volume is piecewise bilinear in the point positions with a division by the cell's density, so the few 1e-3 by which the
    device's bf16 decoder differs from the oracle would move votes across cells and stand in every figure below; taken at the same
    point, the figures are about the loss terms and their backward.  forward_host runs with bf16 = True: its convs round their operands
    where the kernels do.  Then torch Adam on the discriminator for hinge(real, fake = the device's reconstruction or its volume)."""
    from oracle import vae as o_vae
    cfg, B, keys = o["cfg"], o["B"], o["keys"]
    sdt = {k: torch.from_numpy(o["sd"][k]).float().requires_grad_() for k in keys}
    pred_h = o_vae.vae_decode.__wrapped__(sdt, cfg, o["z"])
    pred = pred_h + (pred_dev - pred_h).detach()
    target = o["target"]
    sensor = BU.train_sensor()
    nll = (torch.tensor(WC)[None, :, None, None] * (pred - target).abs()).sum() / B
    out = dict(l1=float(nll.detach()))
    w_bev, disc_bev = kw.get("bev_rec_weight", 0.0), kw.get("disc_bev", False)
    vt = vp = None
    if w_bev > 0 or disc_bev:
        vt, vp = sensor.to_voxel_host(target, tables="library").detach(), sensor.to_voxel_host(pred, tables="library")
        out["occupied"] = int((vp[:, 0] > 0).sum())
    if w_bev > 0:
        bev = (vt[:, :1] - vp[:, :1]).abs().sum()
        out["bev_rec"], out["cells"] = float(bev.detach().double()), int(((vt[:, 0] > 0) | (vp[:, 0] > 0)).sum())
        nll = nll + (w_bev / B) * bev
    total = nll
    if "dstate" in kw:
        dstate = kw["dstate"]
        real, fake = (vt, vp) if disc_bev else (target, pred)
        g_loss = -torch.mean(D.forward_host(dstate, fake, training=True, bf16=True))
        last = sdt["decoder.conv_out.weight"]
        d_weight = D.adaptive_weight_host(torch.autograd.grad(nll, last, retain_graph=True)[0],
                                          torch.autograd.grad(g_loss, last, retain_graph=True)[0], 0.5)
        total = nll + d_weight * g_loss
        out.update(g_loss=float(g_loss.detach()), d_weight=float(d_weight))
        parts = [torch.autograd.grad(t, pred, retain_graph=True)[0].sum((0, 2, 3)) for t in (nll, d_weight * g_loss)]
        out["bias_conditioning"] = float((parts[0] + parts[1]).norm() / (parts[0].norm() + parts[1].norm()))
        dp = {k: torch.nn.Parameter(v.clone()) for k, v in dstate.items() if not k.endswith(D.BUFFER_SUFFIXES)}
        buffers = {k: v.clone() for k, v in dstate.items() if k.endswith(D.BUFFER_SUFFIXES)}
        opt = torch.optim.Adam(list(dp.values()), lr=o["lr"], betas=(0.9, 0.999), eps=1e-8)
        st = dict(dp, **buffers)
        D.forward_host(st, fake.detach(), True, True, buffers)
        D.hinge_d_loss_host(D.forward_host(st, real, True, True, buffers), D.forward_host(st, fake.detach(), True, True, buffers)).backward()
        opt.step()
        out["dparams"] = {k: v.detach() for k, v in dp.items()}
    out["grads"] = dict(zip(keys, torch.autograd.grad(total, [sdt[k] for k in keys])))
    vp_ = [torch.nn.Parameter(torch.from_numpy(o["sd"][k]).float().clone()) for k in keys]
    opt = torch.optim.Adam(vp_, lr=o["lr"], betas=(0.9, 0.999), eps=1e-8)
    for p, k in zip(vp_, keys):
        p.grad = out["grads"][k].clone()
    opt.step()
    out["params"] = {k: p.detach() for p, k in zip(vp_, keys)}
    return out


def _adam_figures(got, want, init, names, lr):
    d = torch.cat([(got[k].cpu() - want[k]).reshape(-1) for k in names]).abs()
    upd = torch.cat([(want[k] - init[k]).reshape(-1) for k in names])
    return float((d > 0.5 * lr).float().mean()), float(d.norm() / upd.norm())


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_train_step_with_bev_terms_matches_autograd_and_adam(variant, capsys):
    """One train_step of VAEDecoderTrainer with bev_rec_weight alone (no discriminator), disc_bev alone, and both: last_bev_rec,
    last_g_loss, last_d_weight and every VAE parameter gradient against host_step; the VAE's parameters (without a discriminator) or the
    discriminator's (with one) after the step against torch Adam.  The gates are STEP_GATES of tests/test_discriminator_gpu.py,
    unchanged.  last_bev_rec: both sides sum |log(d + 1)| differences of fp32 volumes of the same image in fp64; per cell that either
    side occupies the device's logf and the order of its atomics stand for at most the 2e-5 + bound_d of test_hip_splat_cell_by_cell,
    taken here as 4e-5 per such cell (fewer than 64 votes a cell: bound_d < 64 u d < 2e-5).

    Measured on an MI355X (gate):
      bev_rec   grad_worst 0.0111 (0.06), grad_all 0.0015 (0.05), adam_beyond_half_step 0.0026 (0.031), adam_rel 0.101 (0.49)
      disc_bev  grad_worst 0.0143, grad_all 0.0048, g_loss 0.00023 (0.0034), d_weight 0.00015 (0.0046), adam_beyond_half_step 0.0012,
                adam_rel 0.070
      both      grad_worst 0.0139, grad_all 0.0057, g_loss 0.00028, d_weight 0.0020, adam_beyond_half_step 0.0059, adam_rel 0.154
    (worst gradient: decoder.up_blocks.0.upsamplers.0.conv.bias, as in the existing adversarial test).  Piece by piece at this case:
    V(pred) against to_voxel_host 4e-8, d nll / d pred 4e-8, the host's dvoxel through the device's to_voxel_backward 3e-8; the
    PatchGAN's input gradient dvoxel is 0.08 from forward_host(bf16=True)'s, the level tests/test_discriminator_gpu.py records for
    that network (g_dx), and 0.009 in the image gradient of g_loss behind the backward."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    from tests.test_discriminator_gpu import STEP_GATES, _param_errors
    o = train_case()
    kw = dict(VARIANTS[variant])
    disc = None
    if kw.get("disc_bev"):
        disc = D.PatchDiscriminator(state=o["dstate"], lr=o["lr"])
    tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=o["lr"], discriminator=disc, disc_start=0, bev=BU.train_sensor(), **kw)
    snap = {}
    step = tr.optimizer_step

    def keep_then_step():
        snap.update({n: tr.g[n].cpu().clone() for n in tr.names})
        return step()
    tr.optimizer_step = keep_then_step
    loss = tr.train_step(o["z"].cuda(), o["target"].cuda())
    torch.cuda.synchronize()
    pred_dev = tr.sample_nchw().cpu()
    ref = host_step(o, dict(kw, **({"dstate": o["dstate"]} if disc is not None else {})), pred_dev)
    assert ref["occupied"] >= 100                                                         # the reconstruction lies inside the volume
    assert ref.get("bias_conditioning", 1.0) >= 0.5                                       # (train_case: conv_out.bias is no cancelling sum)
    fig = {}
    w, n, a = _param_errors(snap, ref["grads"], tr.names)
    fig.update(grad_worst=w, grad_all=a)
    init = {k: torch.from_numpy(o["sd"][k]).float() for k in o["keys"]}
    if "bev_rec_weight" in kw:
        got = float(tr.last_bev_rec)
        assert abs(got - ref["bev_rec"]) <= 4e-5 * ref["cells"], (got, ref["bev_rec"])
        assert ref["bev_rec"] > 1.0 and abs(float(loss) - (ref["l1"] + BEV_W / o["B"] * ref["bev_rec"])) <= 1e-5 * float(loss)
    else:
        assert tr.last_bev_rec is None
    if disc is not None:
        fig["g_loss"] = abs(float(tr.last_g_loss) - ref["g_loss"]) / abs(ref["g_loss"])
        fig["d_weight"] = abs(float(tr.last_d_weight) - ref["d_weight"]) / ref["d_weight"]
        assert tr.global_step == 1 and disc.global_step == 1 and int(disc.buffers["main.3.num_batches_tracked"]) == 3
        fig["adam_beyond_half_step"], fig["adam_rel"] = _adam_figures(disc.state_dict(), ref["dparams"], o["dstate"], disc.names, o["lr"])
    else:
        assert tr.last_g_loss is None and tr.last_d_weight is None and tr.last_disc is None
        fig["adam_beyond_half_step"], fig["adam_rel"] = _adam_figures(tr.state_dict(), ref["params"], init, tr.names, o["lr"])
    with capsys.disabled():
        print(f"\n{variant}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()) + f"; worst gradient {n}")
    bad = {k: (v, STEP_GATES[k]) for k, v in fig.items() if not v <= STEP_GATES[k]}
    assert not bad, bad


def _bits(tr):
    return [t.cpu().clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


@pytest.mark.parametrize("which", ["decoder", "all"])
def test_defaults_leave_the_step_bit_identical(which):
    """Two deterministic trainers, one of them given bev= with both switches off, over the adversarial phase boundary: the same bits."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    o = train_case()
    g = torch.Generator().manual_seed(5)
    batches = [(torch.rand(2, 2, 32, 8, generator=g), torch.randn(2, 4, 16, 4, generator=g)) for _ in range(3)]
    assert o["cfg"].z_channels == 4 and o["cfg"].downscale == 2
    runs = []
    for kw in ({}, dict(bev=BU.train_sensor(), bev_rec_weight=0.0, disc_bev=False)):
        disc = D.PatchDiscriminator(D.DiscriminatorConfig(2, 16, 1), seed=3, lr=1e-3, deterministic=True)
        if which == "all":
            tr = VAETrainer(o["cfg"], o["sd"], lr=1e-3, deterministic=True, discriminator=disc, disc_start=1, **kw)
            losses = [float(tr.train_step(x.cuda(), noise=n.cuda())) for x, n in batches]
        else:
            tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=1e-3, deterministic=True, discriminator=disc, disc_start=1, **kw)
            losses = [float(tr.train_step(n.cuda(), x.cuda())) for x, n in batches]
        assert tr.last_bev_rec is None and tr.last_disc is not None
        runs.append((losses, _bits(tr) + _bits(disc)))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_refusals():
    from rangeldm_amd.metakernel import MetaKernelConfig, MetaKernelDiscriminator
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    o = train_case()
    cfg, sd, bev = o["cfg"], o["sd"], BU.train_sensor()
    patch = D.PatchDiscriminator(DCFG, seed=1)
    for cls in (VAEDecoderTrainer, VAETrainer):
        with pytest.raises(ValueError, match="bev="):
            cls(cfg, sd, bev_rec_weight=1.0)
        with pytest.raises(ValueError, match="bev="):
            cls(cfg, sd, discriminator=patch, disc_bev=True)
        with pytest.raises(NotImplementedError, match="atomics"):
            cls(cfg, sd, bev=bev, bev_rec_weight=1.0, deterministic=True)
        with pytest.raises(NotImplementedError, match="atomics"):
            cls(cfg, sd, bev=bev, discriminator=patch, disc_bev=True, deterministic=True)
        with pytest.raises(ValueError, match="PatchDiscriminator"):
            cls(cfg, sd, bev=bev, discriminator=MetaKernelDiscriminator(MetaKernelConfig(in_channels=2, ndf=16), seed=1), disc_bev=True)
        with pytest.raises(ValueError, match="PatchDiscriminator"):
            cls(cfg, sd, bev=bev, disc_bev=True)
        with pytest.raises(ValueError, match="beam"):
            cls(cfg, sd, bev=BU.bev_sensor(*BU.SPLAT_GRIDS[0], "linear"), bev_rec_weight=1.0)
        cls(cfg, sd, bev=None, bev_rec_weight=0.0, disc_bev=False, deterministic=True)       # the defaults refuse nothing


def test_state_round_trip_with_a_bev_discriminator(tmp_path):
    from rangeldm_amd.vae_training import VAETrainer
    o = train_case()
    g = torch.Generator().manual_seed(9)
    images = [(o["target"] + 0.01 * torch.randn(o["target"].shape, generator=g)).contiguous() for _ in range(3)]

    def make(seed):
        disc = D.PatchDiscriminator(DCFG, seed=seed, lr=1e-3)
        return VAETrainer(o["cfg"], o["sd"], lr=1e-3, discriminator=disc, disc_start=1, bev=BU.train_sensor(), bev_rec_weight=BEV_W, disc_bev=True)
    a = make(3)
    for x in images[:2]:
        a.train_step(x.cuda(), sample_posterior=False)
    assert a.last_disc is not None and a.discriminator.global_step == 2 and float(a.last_bev_rec) > 0
    path = str(tmp_path / "state.pt")
    a.save_state(path)
    b = make(8)
    b.load_state(path)
    assert b.global_step == 2 and b.discriminator.global_step == 2
    for x, y in zip(_bits(a) + _bits(a.discriminator), _bits(b) + _bits(b.discriminator)):
        assert torch.equal(x, y)
    assert all(torch.equal(a.discriminator.buffers[k], b.discriminator.buffers[k]) for k in a.discriminator.buffers)
    la, lb = float(a.train_step(images[2].cuda(), sample_posterior=False)), float(b.train_step(images[2].cuda(), sample_posterior=False))
    assert np.isfinite(la) and abs(la - lb) <= 1e-3 * abs(la)          # (the splat's atomics: the continuation is not bit-reproducible)


def test_command_line_runs_the_bev_terms(tmp_path, capsys):
    """python -m rangeldm_amd.train_vae --discriminator patchgan --disc-bev --bev-rec-weight 1 --bev-grid 1 32 32, in process, on images
    of height 64 (the KITTI-360 sensor) and width 32: every JSON line carries bev_rec; without the flags the keys are what they were."""
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae_training import save_vae_dir
    from tests.test_vae_training_gpu import TALL
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    src, out, out2 = tmp_path / "src", tmp_path / "out", tmp_path / "out2"
    save_vae_dir(str(src), cfg, sd)
    base = ["--weights", str(src), "--steps", "2", "--batch-size", "2", "--lr", "1e-3", "--log-every", "1", "--seed", "4"]
    CLI.main(base + ["--out", str(out), "--discriminator", "patchgan", "--disc-start", "1", "--disc-bev", "--bev-rec-weight", "1",
                     "--bev-grid", "1", "32", "32"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [1, 2]
    assert set(lines[0]) == {"step", "loss", "mae", "bev_rec"}
    assert set(lines[1]) == {"step", "loss", "mae", "bev_rec", "g_loss", "d_weight", "disc_loss", "logits_real", "logits_fake"}
    assert all(np.isfinite(v) for l in lines for k, v in l.items() if k != "mae") and all(l["bev_rec"] >= 0 for l in lines)
    st = torch.load(str(out / "discriminator.pt"), map_location="cpu", weights_only=True)
    assert st["global_step"] == 2 and (out / "vae").is_dir()
    CLI.main(base + ["--out", str(out2)])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert all(set(l) == {"step", "loss", "mae"} for l in lines)
