"""GPU: the Meta-Kernel layer's kernels (rangeldm_amd/csrc/train_meta.hip) exactly on integer-valued operands against their fp64
host statements; the boundary rules; the refusals; the network against the reference's recording (tests/golden/metakernel.npz);
MetaKernelDiscriminator's step, state and its place in the VAE trainers and the command line.

Gates of the network and trainer tests: twice the distance of forward_host(bf16=True) -- the host network with the MFMA operands
rounded where the kernels round them -- from the same reference, computed on the CPU inside the test and printed beside the device's
figure.  That distance is what bf16 operands cost; the factor 2 allows for a different summation order.  No gate comes from a
device run."""
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import discriminator as D
from rangeldm_amd import metakernel as MK
from tests.disc_util import META as U
from tests.disc_util import mode
from tests.disc_util import param_errors as _param_errors
from tests.hip_util import assert_bitexact
from tests.meta_util import exact_layer_case
from tests.test_discriminator_gpu import _vae_batch, _vae_bits

pytestmark = pytest.mark.gpu

# The GEMM tile of train_meta.hip is 64 x 64 with 32-deep K chunks.  (2, 16, 6, 16 -> 80) stride 1 has 150 pixels (three M tiles of
# the coov GEMM, 38 of the MLP's), N in two tiles, 16 C = 256 = eight K chunks; (3, 32, 12, 2 -> 16) has 288 pixels and the fp32 MLP.
LAYER_CASES = [
    # (B, W, H, C, N, stride)
    (2, 8, 6, 2, 16, 2),
    (2, 8, 6, 16, 32, 2),
    (1, 6, 4, 32, 16, 1),
    (2, 4, 3, 16, 1, 1),            # odd H, N = 1
    (2, 16, 6, 16, 80, 1),
    (3, 32, 12, 2, 16, 2),
    (1, 7, 5, 16, 16, 2),           # odd extents at stride 2: 7 -> 3, 5 -> 2
]


def _dev(c, *keys):
    return [c[k].cuda() for k in keys]


def _run_layer(c, stride, params=True, want_input=True):
    x, r, tab, w1, b1, w2, b2, coov, bias, dy, drn = _dev(c, "x", "r", "tables", "w1", "b1", "w2", "b2", "coov", "bias", "dy", "dr_next")
    y, rn, saved = MK.meta_forward(x, r, tab, w1, b1, w2, b2, coov, bias, stride)
    grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2, coov, bias)] if params else None
    dx, dr = MK.meta_backward(x, dy, tab, w1, b1, w2, coov, saved, stride, grads, want_input=want_input, dr_next=drn if want_input else None)
    return y, rn, saved, grads, dx, dr


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_exact(case, det):
    B, W, H, Cc, N, stride = case
    c = exact_layer_case(*case)
    ref = c["ref"]
    what = f"{case} {'deterministic' if det else 'default'}"
    f = lambda a: torch.from_numpy(np.asarray(a)).float()        # noqa: E731
    with mode(det):
        y, rn, saved, grads, dx, dr = _run_layer(c, stride)
        pe, src, m = saved
        assert_bitexact(pe.cpu(), f(ref["pe"]), names=("row", "e"), what="pe " + what)
        assert torch.equal(src.cpu(), torch.from_numpy(ref["src"]))
        assert_bitexact(m.cpu(), f(ref["m"]), names=("row", "c"), what="m " + what)
        assert_bitexact(y.cpu(), f(ref["y"]), names=("image", "w", "h", "n"), what="output " + what)
        assert_bitexact(rn.cpu(), f(ref["r_next"]), names=("image", "w", "h"), what="returned r " + what)
        assert_bitexact(dx.cpu(), f(ref["dx"]), names=("image", "w", "h", "c"), what="dx " + what)
        assert_bitexact(dr.cpu(), f(ref["dr"]), names=("image", "w", "h"), what="dr " + what)
        for got, k in zip(grads, ("dw1", "db1", "dw2", "db2", "dcoov", "dbias")):
            assert_bitexact(got.cpu(), f(ref[k]).reshape(got.shape), names=("n", "k"), what=f"{k} {what}")
        # the input gradient alone: the same dx and dr, no parameter gradient asked for; the parameters alone: the same six
        _, _, _, none, dx2, dr2 = _run_layer(c, stride, params=False)
        assert none is None and torch.equal(dx2, dx) and torch.equal(dr2, dr)
        _, _, _, grads3, dx3, dr3 = _run_layer(c, stride, want_input=False)
        assert dx3 is None and dr3 is None and all(torch.equal(a, b) for a, b in zip(grads3, grads))


# ---- boundary behaviour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_w_wraps(stride):
    """An input that is non-zero in column W - 1 alone changes output column 0 (tap j = 0 of column 0 reads column -1 = W - 1): the
    opposite of test_conv4_does_not_wrap_w.  And the gradient of output column 0 reaches input column W - 1."""
    case = (1, 8, 6, 16, 16, stride)
    c = dict(exact_layer_case(*case))
    x = torch.zeros_like(c["x"])
    x[:, 7] = 1.0
    c["x"], c["bias"] = x, torch.zeros_like(c["bias"])
    n = {k: v.numpy() for k, v in c.items() if k != "ref"}
    dy = torch.zeros_like(c["dy"])
    dy[:, 0] = 5
    c["dy"] = dy
    ref = MK.layer_host(n["x"], n["r"], n["tables"], n["w1"], n["b1"], n["w2"], n["b2"], n["coov"], n["bias"], stride, dy=dy.numpy(),
                        dr_next=n["dr_next"])
    y, _, _, _, dx, _ = _run_layer(c, stride)
    assert_bitexact(y.cpu(), torch.from_numpy(ref["y"]).float(), names=("image", "w", "h", "n"), what="W seam")
    assert float(torch.from_numpy(ref["y"])[:, 0].abs().max()) > 0.0 and float(y[:, 0].abs().max()) > 0.0
    # columns whose window does not hold column 7 stay zero (stride 2: outputs 1 and 2 read columns 1 .. 4 and 3 .. 6)
    assert float(y[:, 1 if stride == 2 else 2].abs().max()) == 0.0
    assert_bitexact(dx.cpu(), torch.from_numpy(ref["dx"]).float(), names=("image", "w", "h", "c"), what="dx at the W seam")
    assert float(dx[:, 7].abs().max()) > 0.0


def test_border_rows_and_centre_tap():
    """Outside [0, H): x = 0 (src = -1) and r = 100; r_c is tap (2, 2) of the window."""
    B, W, H, Cc, N, stride = case = (2, 8, 6, 16, 16, 2)
    c = exact_layer_case(*case)
    _, rn, (pe, src, _), _, _, _ = _run_layer(c, stride, params=False)
    pe, src, rn = pe.cpu().reshape(B, 4, 3, 4, 4, 3), src.cpu().reshape(B, 4, 3, 4, 4), rn.cpu()
    r, tab = c["r"], c["tables"].reshape(4, 4, 4)
    assert bool((src[:, :, 0, 0, :] == -1).all()) and bool((src[:, :, 1:, 0, :] >= 0).all())      # row -1 is read by ho = 0, i = 0 alone
    assert bool((src[:, :, :, 1:3, :] >= 0).all())
    centre = r[:, [1, 3, 5, 7]][:, :, [1, 3, 5]]
    assert torch.equal(rn, centre)
    ca, sa, ci, si = tab
    want = torch.stack([(100.0 * ca[0]) * ci[0] - centre[:, :, 0, None], ((100.0 * ca[0]) * si[0]).expand(B, 4, 4),
                        (100.0 * sa[0]).expand(B, 4, 4)], -1)
    assert torch.equal(pe[:, :, 0, 0], want)
    # tap (2, 2) is the centre itself: pe0 = r_c (ca ci - 1) there
    assert torch.equal(pe[:, :, :, 2, 2, 0], (centre * ca[2, 2]) * ci[2, 2] - centre)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_shapes_without_an_instance_are_refused():
    for shape, N, stride in (((1, 8, 6, 3), 16, 2), ((1, 8, 6, 24), 16, 2), ((1, 8, 6, 16), 8, 2), ((1, 8, 6, 16), 16, 3),
                             ((1, 1, 6, 16), 16, 1), ((0, 8, 6, 16), 16, 1)):
        with pytest.raises(ValueError, match="no Meta-Kernel layer instance"):
            MK.layer_desc(shape, N, stride)
    MK.layer_desc((1, 8, 6, 2), 1, 1)
    with pytest.raises(NotImplementedError, match="log"):
        MK.MetaKernelDiscriminator(MK.MetaKernelConfig(log=True))
    with pytest.raises(NotImplementedError, match="log"):
        MK.MetaKernelDiscriminator(dict(ndf=16, log=True))


# ---- the network against the golden ------------------------------------------------------------------------------------------------
GATE_KEYS = ("logits", "d_loss", "g_loss", "d_worst", "d_all", "d_dx0", "d_dx1", "g_worst", "g_all", "g_dx0", "g_dx1", "running")


def _dx_figures(tag, got, ref):
    """The input gradients per channel: channel 0 carries the range path's gradient as well."""
    return {f"{tag}_dx{ch}": max(U.rel(got[k][:, ch], ref[k][:, ch]) for k in ("real", "fake") if k in ref) for ch in (0, 1)}


def network_figures(ndf, W, H, det=False):
    """One run of the golden's sequence on the device -> (the device's figures, forward_host(bf16=True)'s): each figure is a distance
    from the reference's recording (through forward_host in fp32, which tests/test_metakernel_host.py ties to the golden arrays)."""
    return U.network_figures(ndf, W, H, _dx_figures, det)


@pytest.mark.parametrize("ndf,W,H", U.CASES)
def test_network_matches_the_golden(ndf, W, H):
    fig, floor = network_figures(ndf, W, H)
    print(f"ndf {ndf} {W}x{H}: " + ", ".join(f"{k} {fig[k]:.3g} (bf16 host {floor[k]:.3g})" for k in GATE_KEYS)
          + f"; worst d {fig['d_worst_name']}, worst g {fig['g_worst_name']}")
    bad = {k: (fig[k], 2 * floor[k]) for k in GATE_KEYS if not fig[k] <= 2 * floor[k]}
    assert not bad, bad


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
def test_discriminator_step_is_bit_reproducible_in_deterministic_mode():
    U.check_step_is_bit_reproducible()


def test_state_round_trip(tmp_path):
    sa, c = U.check_state_round_trip(tmp_path)                      # (a state dict with the reference's keys loads, tables included)
    assert torch.equal(sa["main.5.sin_inc"], U.init(16)["main.5.sin_inc"])
    assert c.cfg.ndf == 16 and c.cfg.n_layers == 3
    assert c.wf == {} and c.wt == {}                                # the kernels read the fp32 masters: no bf16 operand copy, no pack launch


# ---- the adversarial phase of the VAE trainers -------------------------------------------------------------------------------------
# As tests/test_discriminator_gpu.py: SMALL's 32 x 8 images leave room for n_layers = 1 alone (main.0 stride 2, main.2 + BatchNorm
# stride 1, main.5): 32 x 8 -> 16 x 4 -> 15 x 3 -> 14 x 2 logits.
WC = (40.0, 10.0)
MCFG = MK.MetaKernelConfig(2, 16, 1)
_ADV = {}


def _vae_rounding():
    """tools/vae_bf16_floor.py's switch: the oracle's convs with x, w and dy rounded to bf16 (what the VAE's training convs round)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "vae_bf16_floor.py")
    spec = importlib.util.spec_from_file_location("vae_bf16_floor", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._round_convs


def adv_case():
    """Once: the host reference of one adversarial step of VAEDecoderTrainer, twice -- autograd of nll + d_weight g_loss on the oracle
    decoder + forward_host, and torch Adam on the discriminator for hinge(real = target, fake = the oracle's prediction).  `bf16`: the
    emulation of everything the device rounds (the decoder's conv operands as tools/vae_bf16_floor.py rounds them, the discriminator's
    MFMA operands as forward_host(bf16=True) does): what the device is compared with.  `fp32`: plain autograd, what the emulation's
    distance -- the gates -- is measured against."""
    if not _ADV:
        from oracle import vae as o_vae
        from rangeldm_amd.params import vae_param_shapes
        from rangeldm_amd.synth import synth_state_dict
        from tests.test_vae_training_gpu import SMALL
        cfg, B, lr = SMALL, 3, 1e-3
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(7)
        f = cfg.downscale
        z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        keys = [k for k in sd if k.startswith("decoder.")]
        dstate = MK.init_state(MCFG, 3)
        names = MK.trainable_names(MCFG)
        round_convs = _vae_rounding()
        target = None
        for bf16 in (False, True):
            sdt = {k: torch.from_numpy(np.array(sd[k])).float().requires_grad_() for k in keys}
            round_convs(bf16)
            try:
                pred = o_vae.vae_decode.__wrapped__(sdt, cfg, z)
                if target is None:                                  # an L1 target with a sign margin around the fp32 prediction
                    s = torch.randint(0, 2, pred.shape, generator=g).float() * 2 - 1
                    target = (pred.detach() + s * (0.25 + 0.25 * torch.rand(pred.shape, generator=g))).contiguous()
                nll = (torch.tensor(WC)[None, :, None, None] * (pred - target).abs()).sum() / B
                last = sdt["decoder.conv_out.weight"]
                gn = torch.autograd.grad(nll, last, retain_graph=True)[0]
                g_loss = -torch.mean(MK.forward_host(dstate, pred, training=True, bf16=bf16))
                d_weight = D.adaptive_weight_host(gn, torch.autograd.grad(g_loss, last, retain_graph=True)[0], 0.5)
                grads = dict(zip(keys, torch.autograd.grad(nll + d_weight * g_loss, [sdt[k] for k in keys])))
            finally:
                round_convs(False)
            dp = {k: torch.nn.Parameter(dstate[k].clone()) for k in names}
            buffers = {k: v.clone() for k, v in dstate.items() if k not in dp}
            opt = torch.optim.Adam(list(dp.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
            st = dict(dp, **buffers)
            fake = pred.detach()
            MK.forward_host(st, fake, True, bf16, buffers)            # (the generator's pass moved the running statistics first)
            d_loss = D.hinge_d_loss_host(MK.forward_host(st, target, True, bf16, buffers), MK.forward_host(st, fake, True, bf16, buffers))
            d_loss.backward()
            opt.step()
            _ADV["bf16" if bf16 else "fp32"] = dict(d_weight=float(d_weight), g_loss=float(g_loss.detach()), grads=grads,
                                                    d_loss=float(d_loss.detach()), dparams={k: v.detach() for k, v in dp.items()},
                                                    dbuffers=buffers)
        _ADV.update(cfg=cfg, B=B, lr=lr, sd=sd, z=z, target=target, dstate=dstate, keys=keys)
    return _ADV


def _step_figures(o, ref, grads, dparams, dbuffers, d_weight, g_loss, d_loss, names, vae_names):
    """The figures of tests/test_discriminator_gpu.py::adversarial_figures for one result against one reference."""
    w, n, a = _param_errors(grads, ref["grads"], vae_names)
    d = torch.cat([(dparams[k].cpu() - ref["dparams"][k]).reshape(-1) for k in names]).abs()
    upd = torch.cat([(ref["dparams"][k] - o["dstate"][k]).reshape(-1) for k in names])
    return dict(d_weight=abs(d_weight - ref["d_weight"]) / ref["d_weight"], g_loss=abs(g_loss - ref["g_loss"]) / abs(ref["g_loss"]),
                grad_worst=w, grad_all=a, d_loss=abs(d_loss - ref["d_loss"]) / ref["d_loss"],
                adam_beyond_half_step=float((d > 0.5 * o["lr"]).float().mean()), adam_rel=float(d.norm() / upd.norm()),
                running=max(U.rel(dbuffers[k], ref["dbuffers"][k]) for k in dbuffers if k.endswith(("running_mean", "running_var")))), n


STEP_KEYS = ("d_weight", "g_loss", "grad_worst", "grad_all", "d_loss", "running", "adam_beyond_half_step", "adam_rel")


def test_adversarial_step_matches_autograd_and_adam():
    """One adversarial train_step of VAEDecoderTrainer at SMALL with a MetaKernelDiscriminator against torch autograd of nll + d_weight
    g_loss through forward_host(bf16=True) (behind a decoder whose conv operands are rounded as the device's are) and torch Adam; each
    figure's gate is twice the same figure of that bf16 reference against the fp32 one (adv_case)."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    o = adv_case()
    disc = MK.MetaKernelDiscriminator(state=o["dstate"], lr=o["lr"])
    tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=o["lr"], discriminator=disc, disc_start=0)
    assert tr.adversarial()
    snap = {}
    step = tr.optimizer_step

    def keep_then_step():
        snap.update({n: tr.g[n].cpu().clone() for n in tr.names})
        return step()
    tr.optimizer_step = keep_then_step
    tr.train_step(o["z"].cuda(), o["target"].cuda())
    torch.cuda.synchronize()
    assert tr.global_step == 1 and disc.global_step == 1
    got = disc.state_dict()
    assert int(got["main.3.num_batches_tracked"]) == 3             # the generator's pass, then real, then fake
    d_loss = float(tr.last_disc[0])
    fig, worst = _step_figures(o, o["bf16"], snap, got, got, float(tr.last_d_weight), float(tr.last_g_loss), d_loss, disc.names, tr.names)
    e = o["bf16"]
    floor, _ = _step_figures(o, o["fp32"], e["grads"], e["dparams"], e["dbuffers"], e["d_weight"], e["g_loss"], e["d_loss"], disc.names, tr.names)
    print("adversarial step at SMALL: " + ", ".join(f"{k} {fig[k]:.3g} (bf16 host against fp32 {floor[k]:.3g})" for k in STEP_KEYS)
          + f"; worst {worst}")
    bad = {k: (fig[k], 2 * floor[k]) for k in STEP_KEYS if not fig[k] <= 2 * floor[k]}
    assert not bad, bad


@pytest.mark.parametrize("which", ["decoder", "all"])
def test_without_a_discriminator_and_before_disc_start_the_step_is_todays(which):
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    o = adv_case()
    cfg, sd = o["cfg"], o["sd"]
    batches = [_vae_batch(cfg, 2, 80 + i) for i in range(3)]
    runs = []
    for kw in ({}, dict(discriminator="later", disc_start=3)):
        disc = None
        if kw:
            disc = kw["discriminator"] = MK.MetaKernelDiscriminator(state=o["dstate"], deterministic=True)
        if which == "all":
            tr = VAETrainer(cfg, sd, lr=1e-3, deterministic=True, **kw)
            losses = [float(tr.train_step(x.cuda(), noise=n.cuda())) for x, n in batches]
        else:
            tr = VAEDecoderTrainer(cfg, sd, lr=1e-3, deterministic=True, **kw)
            losses = [float(tr.train_step(n.cuda(), x.cuda())) for x, n in batches]
        runs.append((losses, _vae_bits(tr)))
        assert tr.last_disc is None and tr.last_g_loss is None and tr.last_d_weight is None
        if disc is not None:
            assert tr.adversarial() and disc.global_step == 0 and int(disc.buffers["main.3.num_batches_tracked"]) == 0
            assert torch.equal(disc.params.cpu(), torch.cat([o["dstate"][n].reshape(-1) for n in disc.names]))
    assert runs[1][0] == runs[0][0] and all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


def test_trainer_state_carries_the_discriminator(tmp_path):
    from rangeldm_amd.vae_training import VAETrainer
    o = adv_case()
    cfg, sd = o["cfg"], o["sd"]
    batches = [_vae_batch(cfg, 2, 90 + i) for i in range(3)]

    def make(seed):
        return VAETrainer(cfg, sd, lr=1e-3, deterministic=True, disc_start=1,
                          discriminator=MK.MetaKernelDiscriminator(MCFG, seed=seed, lr=1e-3, deterministic=True))
    a = make(3)
    a.train_step(batches[0][0].cuda(), noise=batches[0][1].cuda())
    a.train_step(batches[1][0].cuda(), noise=batches[1][1].cuda())
    path = str(tmp_path / "state.pt")
    a.save_state(path)
    a.train_step(batches[2][0].cuda(), noise=batches[2][1].cuda())
    b = make(5)
    b.load_state(path)
    assert b.global_step == 2 and b.discriminator.global_step == 2
    b.train_step(batches[2][0].cuda(), noise=batches[2][1].cuda())
    for x, y in zip(_vae_bits(a) + _vae_bits(a.discriminator), _vae_bits(b) + _vae_bits(b.discriminator)):
        assert torch.equal(x, y)
    assert all(torch.equal(a.discriminator.buffers[k], b.discriminator.buffers[k]) for k in a.discriminator.buffers)


def test_command_line_runs_the_adversarial_phase(tmp_path, capsys):
    """python -m rangeldm_amd.train_vae --discriminator metakernel, in process: the adversarial JSON keys from the first adversarial
    step on, OUT/discriminator.pt beside OUT/vae/, and --disc-state resumes from it."""
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae_training import save_vae_dir
    from tests.test_vae_training_gpu import TALL
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    src, out, out2 = tmp_path / "src", tmp_path / "out", tmp_path / "out2"
    save_vae_dir(str(src), cfg, sd)
    base = ["--weights", str(src), "--batch-size", "2", "--lr", "1e-3", "--log-every", "1", "--seed", "4", "--discriminator", "metakernel",
            "--disc-start", "1"]
    CLI.main(base + ["--steps", "2", "--out", str(out)])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [1, 2]
    new = {"g_loss", "d_weight", "disc_loss", "logits_real", "logits_fake"}
    assert set(lines[0]) == {"step", "loss", "mae"}
    assert set(lines[1]) == {"step", "loss", "mae"} | new and all(np.isfinite(lines[1][k]) for k in new)
    assert (out / "vae").is_dir() and (out / "discriminator.pt").is_file()
    st = torch.load(str(out / "discriminator.pt"), map_location="cpu", weights_only=True)
    assert st["global_step"] == 2 and list(st["names"]) == MK.trainable_names() and int(st["buffers"]["main.3.num_batches_tracked"]) == 3
    assert "main.0.cos_azi" in st["buffers"]
    CLI.main(base + ["--steps", "1", "--out", str(out2), "--disc-state", str(out / "discriminator.pt")])
    capsys.readouterr()
    st2 = torch.load(str(out2 / "discriminator.pt"), map_location="cpu", weights_only=True)
    assert int(st2["buffers"]["main.3.num_batches_tracked"]) == 3       # (disc_start = 1: the one step of this run is a plain one)
    assert torch.equal(st2["params"], st["params"])
