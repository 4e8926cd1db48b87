"""GPU: VAE decoder fine-tuning (rangeldm_amd/vae_training.py) -- the training kernels at the decoder's beam counts (32 and 64, which
no other test reaches), the L1 loss kernel, the decoder's gradients against torch autograd on the oracle, the optimizer, the hand-over
to the inference VAE and the deterministic mode.

Gradient gates (test_decoder_gradients_match_autograd): relative L2 per parameter (with the floor of tests/test_training.py) and over
the flat gradient buffer, worst of three runs on an MI355X, gated at twice that (rounded up to two digits):

    config   upstream gradient   worst parameter   gate     all parameters   gate
    SMALL    given dpred         1.57e-2           3.2e-2   7.21e-3          1.5e-2
    SMALL    L1 (train_step)     1.95e-2           3.9e-2   7.13e-3          1.5e-2
    TALL     given dpred         1.23e-2           2.5e-2   8.73e-3          1.8e-2
    TALL     L1 (train_step)     1.18e-2           2.4e-2   8.84e-3          1.8e-2

The per-parameter gates are inside the UNet's 4e-2; TALL's whole-buffer gate is looser than the UNet's 1.5e-2.  Its cause is the bf16
rounding of the conv operands alone, through a chain of 26 convs with no attention and no skip concatenations to dilute it: the
oracle on the host with every conv's x, w and dy rounded to bf16 (fp32 accumulation, everything else fp32: tools/vae_bf16_floor.py)
misses plain fp32 autograd by 8.68e-3 over TALL's buffer and 7.26e-3 over SMALL's, with the same worst parameters (1.29e-2 on
up_blocks.2.resnets.1.norm2.weight, 1.32e-2 on up_blocks.0.upsamplers.0.conv.bias) -- the device's figures.  The 1- and 2-channel
GroupNorm groups are not it: GroupNorm is fp32 end to end (test_group_norm_at_decoder_shapes: 1e-4).  Forward: the project's 2e-2
(measured 5.7e-3 SMALL, 6.6e-3 TALL by the same emulation)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as o_ops
from oracle import vae as o_vae
from rangeldm_amd.config import VAEConfig
from rangeldm_amd.params import vae_param_shapes
from rangeldm_amd.synth import synth_state_dict
from tests.hip_util import amax, assert_bitexact, assert_exact_bound, int_grid, rel_l2

pytestmark = pytest.mark.gpu
U = 2.0 ** -5
WC = (40.0, 10.0)
TOL_FWD = 2e-2
TOL_DECODE = 1.2e-2          # tests/test_hip_models.py: one network forward of the inference kernels
SMALL = VAEConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, sample_size=(32, 8))
TALL = VAEConfig(ch=64, ch_mult=(1, 2, 4), num_res_blocks=2, sample_size=(32, 64))
CONFIGS = {"SMALL": (SMALL, 3), "TALL": (TALL, 2)}
#                 (worst parameter, all parameters) for (given dpred, L1)
GATES = {"SMALL": ((3.2e-2, 1.5e-2), (3.9e-2, 1.5e-2)), "TALL": ((2.5e-2, 1.8e-2), (2.4e-2, 1.8e-2))}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


class mode:
    """The library's deterministic switch for the duration of a block."""

    def __init__(self, det):
        self.det = det

    def __enter__(self):
        from rangeldm_amd import train_ops as T
        self.prev = T.deterministic_enabled()
        T.deterministic(self.det)

    def __exit__(self, *exc):
        from rangeldm_amd import train_ops as T
        T.deterministic(self.prev)


# ---- the training convs at the decoder's shapes, exact ------------------------------------------------------------------------------
TALL_CASES = [
    # (B, Cin, N, W, H, taps, stride, mode)
    (1, 64, 64, 8, 64, 9, 1, 0),        # 3x3 64 -> 64 on 64 beams
    (2, 128, 128, 8, 32, 9, 1, 0),      # 3x3 128 -> 128 on 32 beams
    (1, 128, 128, 8, 32, 9, 1, 1),      # up-sampler to 16 x 64 (sum2x2 in the data gradient)
    (1, 256, 256, 8, 16, 9, 1, 1),      # up-sampler to 16 x 32
    (1, 64, 2, 8, 64, 9, 1, 0),         # conv_out
    (1, 128, 64, 8, 64, 1, 1, 0),       # 1x1 shortcut on 64 beams
    (1, 4, 256, 8, 16, 9, 1, 0),        # conv_in
    (3, 64, 64, 24, 64, 9, 1, 0),       # odd batch, W not a power of two
]
_CONV_REF = {}


def _conv_reference(case):
    """Integer-grid operands (tests/test_train_exact.py's grid: activations / gradients in [-3, 3], weights {-4 .. 4} 2^-5, bias on the
    2^-5 grid) and their fp64 forward / data gradient / weight gradient, once per case."""
    if case not in _CONV_REF:
        B, Cin, N, W, H, taps, stride, md = case
        k = 3 if taps == 9 else 1
        x = int_grid((B, Cin, W, H), 601)
        w = int_grid((N, Cin, k, k), 602, -4, 4, exp=-5)
        bias = int_grid((N,), 603, -64, 64, exp=-5)
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        xin = F.interpolate(x64, scale_factor=2.0, mode="nearest") if md == 1 else x64
        ref = o_ops.circ_conv2d(xin, w64, bias.double(), stride, 1 if taps == 9 else 0)
        dy = int_grid(ref.shape, 605)
        ref.backward(dy.double())
        P = B * ref.shape[2] * ref.shape[3]
        assert_exact_bound(U, (Cin * taps * 4, amax(x) * amax(w)), (1, amax(bias)))
        assert_exact_bound(U, (N * taps * 4, amax(dy) * amax(w)))                             # data gradient (x 4: sum2x2)
        assert_exact_bound(1.0, (P * (4 if md == 1 else 1), amax(dy) * amax(x)))              # dw, bias sums
        _CONV_REF[case] = (x, w, bias, dy, ref.detach(), x64.grad, w64.grad)
    return _CONV_REF[case]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", TALL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_train_conv_at_decoder_shapes_exact(case, det):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, taps, stride, md = case
    x, w, bias, dy, ref, dx_ref, dw_ref = _conv_reference(case)
    what = f"{case} {'deterministic' if det else 'default'}"
    with mode(det):
        wf, wt = T.pack_weights(w.cuda(), taps)
        xd, dyd = nhwc(x), nhwc(dy)
        y = T.conv(xd, wf, N, taps, stride, md, bias=bias.cuda())
        assert_bitexact(nchw(y), ref.float(), what="conv " + what)
        dx = T.sum2x2(T.conv(dyd, wt, Cin, taps, 1, 0)) if md == 1 else T.conv(dyd, wt, Cin, taps, 1, 0)
        assert_bitexact(nchw(dx), dx_ref.float(), what="data gradient " + what)
        dw = torch.zeros_like(w).cuda()
        T.wgrad(dyd, xd, dw, taps, stride, md)
        assert_bitexact(dw.cpu(), dw_ref.float(), names=("n", "cin", "i", "j"), what="wgrad " + what)
        dw2, tot = torch.zeros_like(w).cuda(), torch.zeros(N).cuda()
        T.wgrad_bias(dyd, xd, dw2, taps, stride, md, total=tot)
        assert_bitexact(dw2.cpu(), dw_ref.float(), names=("n", "cin", "i", "j"), what="wgrad_bias " + what)
        assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what="wgrad_bias total " + what)
        rows, tot2 = torch.zeros(B, N).cuda(), torch.zeros(N).cuda()
        T.colsum(dyd, rows=rows, total=tot2)
        assert_bitexact(rows.cpu(), dy.sum((2, 3)), names=("image", "n"), what="colsum rows " + what)
        assert_bitexact(tot2.cpu(), dy.sum((0, 2, 3)), names=("n",), what="colsum total " + what)


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("B,C,W,H", [(1, 64, 8, 64), (2, 128, 8, 32), (1, 32, 8, 8)])
@pytest.mark.parametrize("silu", [True, False])
def test_group_norm_at_decoder_shapes(B, C, W, H, silu, det):
    """The comparison of tests/test_train_ops.py::test_group_norm_forward_backward (fp32 end to end: 2e-5 forward, 1e-4 gradients) at
    64 and 32 beams with 2 and 4 channels per group, and at 1 channel per group."""
    from rangeldm_amd import train_ops as T
    x = (_rnd(B, C, W, H, seed=1) * 2 + 0.5).requires_grad_()
    g = (1 + 0.3 * _rnd(C, seed=2)).requires_grad_()
    b = (0.2 * _rnd(C, seed=3)).requires_grad_()
    ref = o_ops.group_norm_silu(x, g, b, 32, 1e-5, silu)
    dy = _rnd(B, C, W, H, seed=4)
    ref.backward(dy)
    with mode(det):
        xd = nhwc(x.detach())
        y, stats = T.gn_forward(xd, g.detach().cuda(), b.detach().cuda(), 32, 1e-5, silu)
        assert rel_l2(nchw(y), ref.detach()) < 2e-5
        dg, db = torch.zeros(C).cuda(), torch.zeros(C).cuda()
        dx = T.gn_backward(xd, nhwc(dy), stats, g.detach().cuda(), b.detach().cuda(), 32, silu, dg, db)
        assert rel_l2(nchw(dx), x.grad) < 1e-4
        assert rel_l2(dg.cpu(), g.grad) < 1e-4 and rel_l2(db.cpu(), b.grad) < 1e-4
        dx2 = T.gn_backward(xd, nhwc(dy), stats, g.detach().cuda(), b.detach().cuda(), 32, silu, dg, db, dx=dx.clone(), accumulate=True)
        assert rel_l2(nchw(dx2), 2 * x.grad) < 1e-4


# ---- the loss kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("shape,wc", [((2, 2, 8, 4), WC), ((3, 2, 5, 64), WC), ((1, 4, 7, 3), (1.5, 0.25, 3.0, 7.0)),
                                      ((5, 2, 32, 64), WC),                  # 80 partials: more than one block of the 4-per-thread kernel
                                      ((3, 2, 7, 3), WC),                    # two channels, 126 elements: no multiple of 4
                                      ((2, 3, 9, 5), (2.0, 1.0, 0.5))])      # three channels: the element-per-thread kernel
def test_l1_matches_its_numpy_statement(shape, wc, det):
    from rangeldm_amd import train_ops as T
    B, Cc, W, H = shape
    g = torch.Generator().manual_seed(21)
    pred = torch.randn(B, W, H, Cc, generator=g)
    target = torch.randn(B, Cc, W, H, generator=g)
    ties = torch.rand(B, W, H, Cc, generator=g) < 0.1                       # planted exact ties
    pred = torch.where(ties, target.permute(0, 2, 3, 1), pred).contiguous()
    assert int(ties.sum()) > 0
    loss_h, dpred_h, sums_h = T.l1_host(pred.numpy(), target.numpy(), wc)
    with mode(det):
        loss, dpred, sums = T.l1(pred.cuda(), target.cuda(), torch.tensor(wc).cuda())
        torch.cuda.synchronize()
    assert np.array_equal(dpred.cpu().numpy().view(np.uint32), dpred_h.view(np.uint32))            # bit for bit
    assert bool((dpred.cpu()[ties] == 0).all()) and int((dpred.cpu() == 0).sum()) == int(ties.sum())
    loss, sums = float(loss), sums.cpu().numpy()
    print(f"l1 {shape} det={det}: loss {loss!r} host {float(loss_h)!r}")
    if det:
        assert loss == float(loss_h)
        assert np.array_equal(sums, sums_h)
    else:
        assert abs(loss - float(loss_h)) <= 1e-12 * float(loss_h)
        assert np.allclose(sums, sums_h, rtol=1e-12, atol=0)


# ---- the decoder against autograd on the oracle --------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_case(name):
    """Once per config: weights, a latent batch, the oracle's prediction, an upstream gradient with its autograd parameter gradients,
    and the L1 target (oracle_pred + s m, s = +-1, m in [0.25, 0.5]) with the L1 loss and its autograd parameter gradients."""
    if name not in _ORACLE:
        cfg, B = CONFIGS[name]
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(7)
        f = cfg.downscale
        z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        dpred = torch.randn(B, cfg.out_channels, *cfg.sample_size, generator=g)
        keys = [k for k in sd if k.startswith("decoder.")]
        sdt = {k: torch.from_numpy(np.array(sd[k])).float().requires_grad_() for k in keys}
        pred = o_vae.vae_decode.__wrapped__(sdt, cfg, z)
        ga = dict(zip(keys, torch.autograd.grad(pred, [sdt[k] for k in keys], grad_outputs=dpred, retain_graph=True)))
        s = torch.randint(0, 2, pred.shape, generator=g).float() * 2 - 1
        m = 0.25 + 0.25 * torch.rand(pred.shape, generator=g)
        target = (pred.detach() + s * m).contiguous()
        wc = torch.tensor(WC)[None, :, None, None]
        loss = (wc * (pred - target).abs()).sum() / B
        gb = dict(zip(keys, torch.autograd.grad(loss, [sdt[k] for k in keys])))
        _ORACLE[name] = dict(cfg=cfg, B=B, sd=sd, z=z, dpred=dpred, pred=pred.detach(), ga=ga, target=target, gb=gb,
                             loss=float((wc.double() * (pred.detach() - target).double().abs()).sum() / B))
    return _ORACLE[name]


def _gradient_errors(tr, gref):
    """(worst per-parameter error, its name, error over the flat buffer): relative L2, per parameter with the floor of
    tests/test_training.py (a gradient whose reference norm is rounding noise is measured against the buffer's rms)."""
    flat_ref = torch.cat([gref[n].reshape(-1) for n in tr.names])
    rms = float(flat_ref.double().norm() / flat_ref.numel() ** 0.5)

    def err(n):
        d = float((tr.g[n].double().cpu() - gref[n].double()).norm())
        return d / (float(gref[n].double().norm()) + 2e-2 * rms * gref[n].numel() ** 0.5)
    worst = max((err(n), n) for n in tr.names)
    return worst[0], worst[1], rel_l2(tr.grads, flat_ref)


def _layers(names):
    """The layers of a parameter-name sequence, consecutive repeats (a layer's weight and bias) folded."""
    out = []
    for n in names:
        layer = n.rsplit(".", 1)[0]
        if not out or out[-1] != layer:
            out.append(layer)
    return out


@pytest.mark.parametrize("name", ["SMALL", "TALL"])
def test_decoder_gradients_match_autograd(name):
    """(a) backward(dpred) for a given upstream gradient, (b) train_step's gradients with the L1 loss, against torch autograd on
    oracle.vae.vae_decode; gates and measured values in the module docstring."""
    from rangeldm_amd import train_ops as T
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    o = oracle_case(name)
    cfg, B = o["cfg"], o["B"]
    (gate_a, gate_a_all), (gate_b, gate_b_all) = GATES[name]
    tr = VAEDecoderTrainer(cfg, o["sd"])
    order = []
    tr._done = lambda *names: order.extend(names)
    pred = tr.forward(o["z"].cuda())
    pred_nchw = tr.sample_nchw().cpu()
    fwd = rel_l2(pred_nchw, o["pred"])
    print(f"{name}: forward rel-L2 {fwd:.3g}")
    assert fwd < TOL_FWD
    # (a)
    tr.backward(nhwc(o["dpred"]))
    torch.cuda.synchronize()
    # backward finishes the layers (a layer's weight and bias together) in the reverse of the parameter order
    assert sorted(order) == sorted(tr.names)
    assert _layers(order) == list(reversed(_layers(tr.names))), "backward does not finish the parameters in reverse tape order"
    wa, na, alla = _gradient_errors(tr, o["ga"])
    print(f"{name} (a) given dpred: worst parameter {wa:.3g} ({na}), all {alla:.3g}")
    assert wa < gate_a and alla < gate_a_all, (wa, na, alla)
    tr.grads.zero_()
    # (b): a second forward (the default mode's sums are not bit-reproducible: this pass's own prediction is the one compared)
    pred = tr.forward(o["z"].cuda())
    pred_nchw = tr.sample_nchw().cpu()
    margin = float((o["pred"] - o["target"]).abs().min())
    dev_err = float((pred_nchw - o["pred"]).abs().max())
    print(f"{name}: min |oracle_pred - target| {margin:.4g}, max |device_pred - oracle_pred| {dev_err:.4g}")
    assert margin > 10 * dev_err                                               # the two sign patterns are provably equal
    loss, dpred, sums = T.l1(pred, o["target"].cuda(), tr.channel_weights)
    assert torch.equal(torch.sign(nchw(dpred)), torch.sign(o["pred"] - o["target"]))
    tr.backward(dpred)
    wb, nb, allb = _gradient_errors(tr, o["gb"])
    print(f"{name} (b) L1: worst parameter {wb:.3g} ({nb}), all {allb:.3g}")
    assert wb < gate_b and allb < gate_b_all, (wb, nb, allb)
    # the loss: |loss_dev - loss_oracle| <= (1 / B) sum wc |pred_dev - pred_oracle|
    bound = float((torch.tensor(WC, dtype=torch.float64)[None, :, None, None] * (pred_nchw - o["pred"]).double().abs()).sum() / B)
    print(f"{name}: loss {float(loss):.6f} oracle {o['loss']:.6f} bound {bound:.3g}")
    assert abs(float(loss) - o["loss"]) <= bound
    n_pix = B * cfg.sample_size[0] * cfg.sample_size[1]
    mae_ref = (pred_nchw - o["target"]).abs().double().sum((0, 2, 3)) / n_pix                # (the fp32 differences, as the kernel takes them)
    assert torch.allclose(sums.cpu() / n_pix, mae_ref, rtol=1e-12, atol=0)


# ---- optimisation -------------------------------------------------------------------------------------------------------------------
def _fixed_batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    f = cfg.downscale
    z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
    target = torch.randn(B, cfg.out_channels, *cfg.sample_size, generator=g)
    return z, target


def test_train_steps_follow_adam():
    """Three steps on one fixed batch against torch.optim.Adam driven by the oracle's autograd gradients: the comparison and gates of
    tests/test_training.py::test_training_steps_follow_adamw_and_reduce_the_loss."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    z, target = _fixed_batch(cfg, 2, 5)
    lr = 1e-3
    tr = VAEDecoderTrainer(cfg, sd, lr=lr)
    params = {k: torch.nn.Parameter(torch.from_numpy(np.array(sd[k])).float()) for k in tr.names}
    opt = torch.optim.Adam(list(params.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    wc = torch.tensor(WC)[None, :, None, None]
    for step in range(1, 4):
        loss = tr.train_step(z.cuda(), target.cuda(), as_float=True)
        opt.zero_grad()
        ref_loss = (wc * (o_vae.vae_decode.__wrapped__(params, cfg, z) - target).abs()).sum() / 2
        ref_loss.backward()
        opt.step()
        ref_loss = float(ref_loss.detach())
        assert abs(loss - ref_loss) < 2e-2 * ref_loss
        got = tr.state_dict()
        d = torch.cat([(got[k] - params[k].detach()).reshape(-1) for k in tr.names]).abs()
        frac = float((d > 0.5 * lr).float().mean())
        upd = torch.cat([(params[k].detach() - torch.from_numpy(np.array(sd[k]))).reshape(-1) for k in tr.names])
        print(f"step {step}: loss {loss:.5f} oracle {ref_loss:.5f}; beyond half a step {frac:.4f}; |d| / |update| {float(d.norm() / upd.norm()):.4f}")
        assert frac < 0.02, (step, frac)
        assert float(d.norm() / upd.norm()) < 0.15
    assert tr.global_step == 3


def test_twenty_steps_reduce_the_loss_and_leave_the_encoder_alone():
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    cfg = SMALL
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth_state_dict(vae_param_shapes(cfg), prefix="vt.").items()}
    before = {k: v.clone() for k, v in sd.items()}
    z, target = _fixed_batch(cfg, 2, 6)
    tr = VAEDecoderTrainer(cfg, sd, lr=1e-3)
    losses = [tr.train_step(z.cuda(), target.cuda(), as_float=True) for _ in range(20)]
    print("losses", [round(v, 3) for v in losses])
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
    full = tr.full_state_dict()
    assert set(full) == set(sd)
    for k, v in before.items():
        assert torch.equal(sd[k], v), k                                         # nothing the caller passed in was written
        if k.startswith("encoder."):
            assert full[k] is sd[k] and torch.equal(full[k], v), k
    assert any(not torch.equal(full[k], before[k]) for k in tr.names)


# ---- hand-over ----------------------------------------------------------------------------------------------------------------------
def test_trained_decoder_reaches_the_inference_vae(tmp_path):
    from rangeldm_amd.vae import AutoencoderKLHIP
    from rangeldm_amd.vae_training import VAEDecoderTrainer, training_step
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    vae = AutoencoderKLHIP(cfg)
    vae.load_state_dict(sd)
    g = torch.Generator().manual_seed(8)
    images = torch.rand(2, cfg.in_channels, *cfg.sample_size, generator=g)
    z = vae.encode(images.cuda()).latent_dist.mode().contiguous()
    before = vae.decode(z).sample.cpu()
    tr = VAEDecoderTrainer(cfg, sd, lr=1e-3)
    for _ in range(2):
        loss = training_step(tr, vae, images, generator=g)
    assert np.isfinite(float(loss))
    tr.load_into(vae)
    after = vae.decode(z).sample.cpu()
    assert rel_l2(after, before) > 1e-3
    trained = tr.full_state_dict()
    ref = o_vae.vae_decode(trained, cfg, z.cpu())
    err = rel_l2(after, ref)
    print(f"decode with the trained weights: rel-L2 {err:.3g} against the oracle, {rel_l2(after, before):.3g} from the untrained decode")
    assert err < TOL_DECODE
    tr.save_pretrained(str(tmp_path))
    again = AutoencoderKLHIP.from_pretrained(str(tmp_path), subfolder="vae").state_dict()
    assert set(again) == set(trained)
    for k, v in trained.items():
        v = v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))
        assert torch.equal(again[k], v.float()), k


def _bits(tr):
    return [t.cpu().clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


def test_saved_state_continues_bit_identically(tmp_path):
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    z, target = _fixed_batch(cfg, 3, 9)
    a = VAEDecoderTrainer(cfg, sd, lr=1e-3, deterministic=True)
    for _ in range(2):
        a.train_step(z.cuda(), target.cuda())
    path = str(tmp_path / "state.pt")
    a.save_state(path)
    for _ in range(2):
        a.train_step(z.cuda(), target.cuda())
    b = VAEDecoderTrainer(cfg, sd, lr=1e-3, deterministic=True)
    b.load_state(path)
    assert b.global_step == 2
    for _ in range(2):
        b.train_step(z.cuda(), target.cuda())
    assert a.global_step == b.global_step == 4
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x, y)


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_deterministic_mode_repeats_bit_for_bit():
    from rangeldm_amd import train_ops as T
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    batches = [_fixed_batch(cfg, 2, 30 + i) for i in range(3)]
    runs = []
    for _ in range(2):
        tr = VAEDecoderTrainer(cfg, sd, lr=1e-3, deterministic=True)
        assert tr.deterministic and not T.deterministic_enabled()
        losses = [float(tr.train_step(z.cuda(), t.cuda())) for z, t in batches]
        assert not T.deterministic_enabled()                                   # (the switch is scoped to the trainer's calls)
        runs.append((losses, _bits(tr)))
    assert runs[0][0] == runs[1][0]
    for x, y in zip(runs[0][1], runs[1][1]):
        assert torch.equal(x, y)
    assert not torch.equal(runs[0][1][0], torch.cat([torch.from_numpy(sd[n]).reshape(-1) for n in tr.names]))


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_command_line_trains_and_writes_a_loadable_vae(tmp_path, capsys):
    """python -m rangeldm_amd.train_vae, in process: --weights DIR --input NPY_DIR (three files, batches of two wrap around) for three
    steps; one JSON line per --log-every steps; OUT/vae/ loads into the inference VAE with the encoder unchanged and the decoder moved."""
    import json
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.vae import AutoencoderKLHIP
    from rangeldm_amd.vae_training import save_vae_dir
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    src, inp, out = tmp_path / "src", tmp_path / "in", tmp_path / "out"
    save_vae_dir(str(src), cfg, sd)
    inp.mkdir()
    g = torch.Generator().manual_seed(12)
    for i in range(3):
        np.save(str(inp / f"{i}.npy"), torch.rand(cfg.in_channels, *cfg.sample_size, generator=g).numpy())
    last = CLI.main(["--weights", str(src), "--input", str(inp), "--out", str(out), "--steps", "3", "--batch-size", "2", "--lr", "1e-3",
                     "--log-every", "2", "--seed", "4"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [2, 3] and lines[-1] == last
    for l in lines:
        assert set(l) == {"step", "loss", "mae"} and len(l["mae"]) == cfg.out_channels
        assert np.isfinite(l["loss"]) and all(np.isfinite(m) and m > 0 for m in l["mae"])
        assert abs(l["loss"] - (WC[0] * l["mae"][0] + WC[1] * l["mae"][1]) * cfg.sample_size[0] * cfg.sample_size[1]) <= 1e-9 * l["loss"]
    got = AutoencoderKLHIP.from_pretrained(str(out), subfolder="vae").state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        same = torch.equal(got[k], torch.from_numpy(v))
        assert same == k.startswith("encoder."), k
