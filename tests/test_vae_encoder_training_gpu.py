"""GPU: training the whole VAE (rangeldm_amd/vae_training.py: VAETrainer) -- the end-only padding of the training convs (the
encoder's two down-samplers) exactly on integer grids, the posterior kernels against their numpy statement, the encoder's and the
decoder's gradients against torch autograd of the whole step on the oracle, the optimizer, the hand-over to the inference VAE, the
deterministic mode and the command line.

Gradient gates (test_whole_vae_gradients_match_autograd): tests/test_vae_training_gpu.py's measure and rule -- relative L2 per
parameter (with that file's floor) and over the flat gradient buffer, worst of three runs on an MI355X, gated at twice that (rounded up
to two digits).  `host` is tools/vae_bf16_floor.py's figure for the same config: the oracle on the host with every conv's operands
rounded to bf16, against plain fp32 autograd.

    config   kl_weight   worst parameter (device / host)   gate     all parameters (device / host)   gate
    SMALL    1e-6        1.99e-2 / 2.04e-2                 4.0e-2   1.11e-2 / 1.11e-2                2.3e-2
    SMALL    1           1.99e-2 / 1.89e-2                 4.0e-2   1.10e-2 / 1.12e-2                2.2e-2
    TALL     1e-6        2.51e-2 / 2.06e-2                 5.1e-2   1.24e-2 / 1.28e-2                2.5e-2

The device sits on the host floor: the whole-buffer errors are the emulation's, and the worst parameters are the same early encoder
GroupNorm layers (SMALL down_blocks.0.resnets.0.norm1.weight on the device, .norm2.bias on the host; TALL
down_blocks.2.resnets.0.norm1.weight at 1.98e-2 in one run, conv_in.bias at 2.51e-2 in another -- the default mode is not reproducible).
They are looser than the decoder's because the gradient reaches the encoder through twice as many bf16 convs.  Forward: the moments
within the project's 2e-2 of oracle.vae.vae_encode (measured 8.3e-3 SMALL, 7.3e-3 TALL; the emulation 8.3e-3, 7.5e-3)."""
import json

import numpy as np
import pytest
import torch

from oracle import ops as o_ops
from oracle import vae as o_vae
from rangeldm_amd.params import vae_param_shapes
from rangeldm_amd.synth import synth_state_dict
from tests.hip_util import amax, assert_bitexact, assert_exact_bound, int_grid, rel_l2
from tests.test_vae_training_gpu import CONFIGS, SMALL, TOL_DECODE, TOL_FWD, U, WC, _bits, _gradient_errors, mode, nchw, nhwc

pytestmark = pytest.mark.gpu
#        (config, kl_weight): (worst parameter, all parameters)
GATES = {("SMALL", 1e-6): (4.0e-2, 2.3e-2), ("TALL", 1e-6): (5.1e-2, 2.5e-2), ("SMALL", 1.0): (4.0e-2, 2.2e-2)}


# ---- the training convs with end-only padding, exact ---------------------------------------------------------------------------------
CONV_CASES = [
    # (B, Cin, N, W, H, stride, pad)
    (1, 64, 64, 8, 64, 2, 1),           # the first down-sampler's 64-beam level
    (2, 128, 128, 8, 32, 2, 1),         # the second down-sampler
    (3, 32, 32, 6, 8, 2, 1),            # odd batch, Wout = 3
    (1, 16, 16, 2, 2, 2, 1),            # one output pixel: the wrap tap lands on column 0, the zero row is always present
    (1, 16, 16, 4, 2, 2, 1),            # Hout = 1
    (1, 2, 64, 8, 64, 1, 0),            # encoder.conv_in
    (1, 256, 8, 8, 16, 1, 0),           # encoder.conv_out
    (1, 64, 64, 8, 64, 2, 0),           # symmetric stride 2: the shift must not leak into the old mode
    (2, 128, 128, 8, 32, 2, 0),
]
_CONV_REF = {}


def _conv_reference(case):
    """tests/test_vae_training_gpu.py's integer grids and their fp64 forward / data gradient / weight gradient, once per case; pad = 1:
    autograd of oracle.ops.downsample_vae."""
    if case not in _CONV_REF:
        B, Cin, N, W, H, stride, pad = case
        x = int_grid((B, Cin, W, H), 601)
        w = int_grid((N, Cin, 3, 3), 602, -4, 4, exp=-5)
        bias = int_grid((N,), 603, -64, 64, exp=-5)
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        ref = o_ops.downsample_vae(x64, w64, bias.double()) if pad else o_ops.circ_conv2d(x64, w64, bias.double(), stride, 1)
        assert tuple(ref.shape) == (B, N, W // stride, H // stride)
        dy = int_grid(ref.shape, 605)
        ref.backward(dy.double())
        P = B * ref.shape[2] * ref.shape[3]
        assert_exact_bound(U, (Cin * 9, amax(x) * amax(w)), (1, amax(bias)))
        assert_exact_bound(U, (N * 9, amax(dy) * amax(w)))                                    # data gradient
        assert_exact_bound(1.0, (P, amax(dy) * amax(x)))                                      # dw, bias sums
        _CONV_REF[case] = (x, w, bias, dy, ref.detach(), x64.grad, w64.grad)
    return _CONV_REF[case]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_train_conv_with_end_padding_exact(case, det):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, stride, pad = case
    x, w, bias, dy, ref, dx_ref, dw_ref = _conv_reference(case)
    what = f"{case} {'deterministic' if det else 'default'}"
    with mode(det):
        wf, wt = T.pack_weights(w.cuda(), 9)
        xd, dyd = nhwc(x), nhwc(dy)
        y = T.conv(xd, wf, N, 9, stride, 0, bias=bias.cuda(), pad=pad)
        assert_bitexact(nchw(y), ref.float(), what="conv " + what)
        dx = T.conv(dyd, wt, Cin, 9, 1, 2 if stride == 2 else 0, pad=pad)
        assert_bitexact(nchw(dx), dx_ref.float(), what="data gradient " + what)
        dw = torch.zeros_like(w).cuda()
        T.wgrad(dyd, xd, dw, 9, stride, 0, pad=pad)
        assert_bitexact(dw.cpu(), dw_ref.float(), names=("n", "cin", "i", "j"), what="wgrad " + what)
        dw2, tot = torch.zeros_like(w).cuda(), torch.zeros(N).cuda()
        T.wgrad_bias(dyd, xd, dw2, 9, stride, 0, total=tot, pad=pad)
        assert_bitexact(dw2.cpu(), dw_ref.float(), names=("n", "cin", "i", "j"), what="wgrad_bias " + what)
        assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what="wgrad_bias total " + what)
        rows, tot2 = torch.zeros(B, N).cuda(), torch.zeros(N).cuda()
        T.colsum(dyd, rows=rows, total=tot2)
        assert_bitexact(rows.cpu(), dy.sum((2, 3)), names=("image", "n"), what="colsum rows " + what)
        assert_bitexact(tot2.cpu(), dy.sum((0, 2, 3)), names=("n",), what="colsum total " + what)


def test_end_padding_is_refused_where_it_has_no_kernel():
    """pad = 1 is the 3x3 stride-2 forward / weight gradient and its zero-insertion data gradient; everything else is a bad conv desc,
    and the fused / all-taps kernels report that they have no such instance."""
    import ctypes as C
    from rangeldm_amd import _lib
    from rangeldm_amd import train_ops as T
    x = torch.zeros(1, 8, 16, 64).cuda()
    w9, _ = T.pack_weights(torch.zeros(64, 64, 3, 3).cuda(), 9)
    w1, _ = T.pack_weights(torch.zeros(64, 64).cuda(), 1)
    for taps, wp, stride, md in ((9, w9, 1, 0), (9, w9, 1, 1), (9, w9, 2, 2), (9, w9, 2, 1), (1, w1, 2, 0), (1, w1, 1, 2)):
        with pytest.raises(RuntimeError, match="bad conv desc"):
            T.conv(x, wp, 64, taps, stride, md, pad=1)
    with pytest.raises(RuntimeError, match="bad conv desc"):
        T.wgrad(torch.zeros(1, 8, 16, 64).cuda(), x, torch.zeros(64, 64, 3, 3).cuda(), 9, 1, 0, pad=1)
    f = _lib.TrainFuseC()
    for stride, md in ((2, 0), (1, 2)):
        d = T.conv_desc(x, 64, 9, stride, md, pad=1)
        assert _lib.lib().rldm_train_conv_fused_ok(C.byref(d), C.byref(f), 0) == 0
        assert _lib.lib().rldm_train_wgrad_fused_ok(C.byref(d), C.byref(f)) == 0
        twin = T.conv_desc(x, 64, 9, stride, md)
        assert _lib.lib().rldm_train_conv_splits(C.byref(d), 0) == _lib.lib().rldm_train_conv_splits(C.byref(twin), 0)
    assert _lib.lib().rldm_train_conv_fused_ok(C.byref(T.conv_desc(x, 64, 9, 1, 0)), C.byref(f), 0) == 1


# ---- the posterior -------------------------------------------------------------------------------------------------------------------
EDGES = (-31.0, -30.0, 20.0, 21.0)
EPS = 16 * 2.0 ** -24                    # four fp32 roundings and a 2-ulp expf, relative to the sum of |terms|


def _posterior_case(B, Z, W, H):
    g = torch.Generator().manual_seed(31)
    m = torch.randn(B, W, H, 2 * Z, generator=g) * 2
    m[0, 0, :4, Z] = torch.tensor(EDGES)
    m[-1, -1, -4:, 2 * Z - 1] = torch.tensor(EDGES)
    return m, torch.randn(B, Z, W, H, generator=g), torch.randn(B, W, H, Z, generator=g)


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("sample", [True, False], ids=["sample", "mode"])
@pytest.mark.parametrize("shape", [(3, 4, 2, 8), (2, 4, 8, 16), (1, 3, 5, 7), (5, 4, 32, 16)])     # 105 .. 10240 elements: 1 .. 40 partials
def test_posterior_matches_its_numpy_statement(shape, sample, det):
    from rangeldm_amd import train_ops as T
    B, Z, W, H = shape
    m, noise, dz = _posterior_case(B, Z, W, H)
    kw = float(np.float32(0.75 / B))
    n_h = noise.numpy() if sample else None
    z_h, kl_h, dm_h = T.gaussian_host(m.numpy(), n_h, dz.numpy(), kw)
    # the sum of the absolute values of every element's terms, in fp64
    m64, dz64 = m.double().numpy(), dz.double().numpy()
    mean, lc = m64[..., :Z], np.clip(m64[..., Z:], -30.0, 20.0)
    n64 = noise.double().numpy().transpose(0, 2, 3, 1) if sample else np.zeros_like(mean)
    z_terms = np.abs(mean) + np.abs(np.exp(0.5 * lc) * n64)
    dm_terms = np.concatenate([np.abs(dz64) + np.abs(kw * mean),
                               np.abs(dz64 * n64 * 0.5 * np.exp(0.5 * lc)) + kw * 0.5 * np.exp(lc) + kw * 0.5], axis=-1)
    with mode(det):
        md, nd, dzd = m.cuda(), (noise.cuda() if sample else None), dz.cuda()
        runs = []
        for _ in range(2):
            z, kl = T.gaussian(md, nd)
            dm = T.gaussian_backward(md, nd, dzd, kw)
            torch.cuda.synchronize()
            runs.append((z.cpu().numpy(), float(kl), dm.cpu().numpy()))
    z, kl, dm = runs[0]
    ez, edm = float((np.abs(z - z_h) / z_terms).max()), float((np.abs(dm - dm_h) / dm_terms).max())
    print(f"posterior {shape} sample={sample} det={det}: z {ez / 2.0 ** -24:.2f} dmoments {edm / 2.0 ** -24:.2f} (units of 2^-24 of the "
          f"terms), kl {kl!r} host {float(kl_h)!r}")
    assert np.all(np.abs(z - z_h) <= EPS * z_terms)
    assert np.all(np.abs(dm - dm_h) <= EPS * dm_terms)
    assert abs(kl - float(kl_h)) <= 1e-6 * float(kl_h)
    for b, w, hs, c in ((0, 0, slice(0, 4), Z), (B - 1, W - 1, slice(H - 4, H), 2 * Z - 1)):
        dl = dm[b, w, hs, c]
        assert dl[0] == 0 and dl[3] == 0 and dl[1] != 0 and dl[2] != 0, dl
    if not sample:
        assert np.array_equal(z, m.numpy()[..., :Z])
    # the planted exp(20) terms dominate that kl: the same moments without them
    plain = m.clone()
    plain[..., Z:] = plain[..., Z:].clamp(-8.0, 8.0)
    with mode(det):
        kl_p = float(T.gaussian(plain.cuda(), None)[1])
    kl_ph = float(T.gaussian_host(plain.numpy())[1])
    assert abs(kl_p - kl_ph) <= 1e-6 * kl_ph, (kl_p, kl_ph)
    if det:
        assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


# ---- the whole VAE against autograd on the oracle -------------------------------------------------------------------------------------
_ORACLE = {}


def _kl(moments, B):
    d = o_vae.DiagonalGaussian(moments)
    return 0.5 * (d.mean ** 2 + torch.exp(d.logvar) - 1 - d.logvar).sum() / B


def oracle_step(name):
    """Once per config: weights, images, noise, the oracle's moments and prediction, the L1 target (oracle_pred + s m, s = +-1, m in
    [0.25, 0.5]: no sign can flip) and the parts of the loss with the autograd graph kept for `oracle_gradients`."""
    if name not in _ORACLE:
        cfg, B = CONFIGS[name]
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(17)
        f = cfg.downscale
        images = torch.rand(B, cfg.in_channels, *cfg.sample_size, generator=g)
        noise = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        sdt = {k: torch.from_numpy(np.array(v)).float().requires_grad_() for k, v in sd.items()}
        moments = o_vae.vae_encode.__wrapped__(sdt, cfg, images)
        z = o_vae.DiagonalGaussian(moments).sample(noise=noise)
        pred = o_vae.vae_decode.__wrapped__(sdt, cfg, z)
        s = torch.randint(0, 2, pred.shape, generator=g).float() * 2 - 1
        m = 0.25 + 0.25 * torch.rand(pred.shape, generator=g)
        target = (pred.detach() + s * m).contiguous()
        rec = (torch.tensor(WC)[None, :, None, None] * (pred - target).abs()).sum() / B
        _ORACLE[name] = dict(cfg=cfg, B=B, sd=sd, sdt=sdt, images=images, noise=noise, moments=moments.detach(), z=z.detach(),
                             pred=pred.detach(), target=target, rec=rec, kl=_kl(moments, B), grads={})
    return _ORACLE[name]


def oracle_gradients(o, kl_weight):
    if kl_weight not in o["grads"]:
        keys = list(o["sdt"])
        o["grads"][kl_weight] = dict(zip(keys, torch.autograd.grad(o["rec"] + kl_weight * o["kl"], [o["sdt"][k] for k in keys],
                                                                   retain_graph=True)))
    return o["grads"][kl_weight]


@pytest.mark.parametrize("name,kl_weight", sorted(GATES), ids=lambda v: str(v))
def test_whole_vae_gradients_match_autograd(name, kl_weight):
    """forward + L1 against the planted target + backward (with kl_weight * kl folded in by the tape) against torch autograd of
    rec + kl_weight * kl on oracle.vae; gates and measured values in the module docstring.  kl_weight = 1 makes the KL path through the
    encoder visible in the total."""
    from rangeldm_amd import train_ops as T
    from rangeldm_amd.vae_training import VAETrainer
    o = oracle_step(name)
    cfg, B = o["cfg"], o["B"]
    gate, gate_all = GATES[(name, kl_weight)]
    tr = VAETrainer(cfg, o["sd"], kl_weight=kl_weight)
    assert sorted(tr.names) == sorted(o["sd"])
    order = []
    tr._done = lambda *names: order.extend(names)
    pred = tr.forward(o["images"].cuda(), o["noise"].cuda())
    fwd_m, fwd_p = rel_l2(tr.moments().cpu(), o["moments"]), rel_l2(tr.sample_nchw().cpu(), o["pred"])
    print(f"{name}: moments rel-L2 {fwd_m:.3g}, reconstruction rel-L2 {fwd_p:.3g}")
    assert fwd_m < TOL_FWD
    assert tuple(tr.latents().shape) == tuple(o["z"].shape)
    pred_nchw = tr.sample_nchw().cpu()
    margin = float((o["pred"] - o["target"]).abs().min())
    dev_err = float((pred_nchw - o["pred"]).abs().max())
    print(f"{name}: min |oracle_pred - target| {margin:.4g}, max |device_pred - oracle_pred| {dev_err:.4g}")
    assert dev_err < margin                                                    # the two sign patterns are provably equal
    rec, dpred, _ = T.l1(pred, o["target"].cuda(), tr.channel_weights)
    assert torch.equal(torch.sign(nchw(dpred)), torch.sign(o["pred"] - o["target"]))
    tr.backward(dpred)
    torch.cuda.synchronize()
    assert sorted(order) == sorted(tr.names)
    gref = oracle_gradients(o, kl_weight)
    worst, wname, err_all = _gradient_errors(tr, gref)
    enc = [n for n in tr.names if n.startswith("encoder.")]
    enc_all = rel_l2(torch.cat([tr.g[n].reshape(-1) for n in enc]), torch.cat([gref[n].reshape(-1) for n in enc]))
    if kl_weight == 1.0:
        # the KL path is visible at this weight: without it encoder.conv_out's gradient would miss the gate on its own
        n, g0 = "encoder.conv_out.weight", oracle_gradients(o, 1e-6)
        assert rel_l2(g0[n], gref[n]) > gate, "kl_weight = 1 does not show the KL path"
    print(f"{name} kl_weight {kl_weight:g}: worst parameter {worst:.3g} ({wname}), all {err_all:.3g}, encoder alone {enc_all:.3g}")
    assert worst < gate and err_all < gate_all, (worst, wname, err_all)
    kl_ref = float(o["kl"].detach())
    print(f"{name}: kl {float(tr.last_kl):.6f} oracle {kl_ref:.6f}")
    assert abs(float(tr.last_kl) - kl_ref) < TOL_FWD * kl_ref


def test_decoder_gradients_equal_the_decoder_trainers_bit_for_bit():
    """Deterministic mode, the same z and the same dpred: the decoder half of VAETrainer is VAEDecoderTrainer's tape (plus conv_in's data
    gradient, which no parameter gradient reads)."""
    from rangeldm_amd import train_ops as T
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    o = oracle_step("SMALL")
    a = VAETrainer(o["cfg"], o["sd"], deterministic=True)
    pred = a.forward(o["images"].cuda(), o["noise"].cuda())
    with mode(True):
        _, dpred, _ = T.l1(pred, o["target"].cuda(), a.channel_weights)
    a.backward(dpred)
    b = VAEDecoderTrainer(o["cfg"], o["sd"], deterministic=True)
    pred_b = b.forward(a.latents())
    assert torch.equal(pred_b, pred)
    b.backward(dpred)
    torch.cuda.synchronize()
    for n in b.names:
        assert torch.equal(a.g[n], b.g[n]), n
    assert all(float(a.g[n].abs().max()) > 0 for n in a.names if n.endswith(".weight"))


# ---- optimisation -------------------------------------------------------------------------------------------------------------------
def _fixed_batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    f = cfg.downscale
    images = torch.rand(B, cfg.in_channels, *cfg.sample_size, generator=g)
    return images, torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)


def _oracle_loss(params, cfg, images, noise, kl_weight):
    B = images.shape[0]
    moments = o_vae.vae_encode.__wrapped__(params, cfg, images)
    pred = o_vae.vae_decode.__wrapped__(params, cfg, o_vae.DiagonalGaussian(moments).sample(noise=noise))
    return (torch.tensor(WC)[None, :, None, None] * (pred - images).abs()).sum() / B + kl_weight * _kl(moments, B)


def test_train_steps_follow_adam():
    """Three steps on one fixed batch against torch.optim.Adam driven by the oracle's autograd gradients of the whole step: the
    comparison and gates of tests/test_vae_training_gpu.py::test_train_steps_follow_adam."""
    from rangeldm_amd.vae_training import VAETrainer
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    images, noise = _fixed_batch(cfg, 2, 5)
    lr = 1e-3
    tr = VAETrainer(cfg, sd, lr=lr)
    params = {k: torch.nn.Parameter(torch.from_numpy(np.array(sd[k])).float()) for k in tr.names}
    opt = torch.optim.Adam(list(params.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    for step in range(1, 4):
        loss = tr.train_step(images.cuda(), noise=noise.cuda(), as_float=True)
        opt.zero_grad()
        ref_loss = _oracle_loss(params, cfg, images, noise, tr.kl_weight)
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


def test_twenty_steps_reduce_the_loss_and_move_the_encoder():
    from rangeldm_amd.vae_training import VAETrainer
    cfg = SMALL
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth_state_dict(vae_param_shapes(cfg), prefix="vt.").items()}
    before = {k: v.clone() for k, v in sd.items()}
    images, noise = _fixed_batch(cfg, 2, 6)
    tr = VAETrainer(cfg, sd, lr=1e-3)
    losses = [tr.train_step(images.cuda(), noise=noise.cuda(), as_float=True) for _ in range(20)]
    print("losses", [round(v, 3) for v in losses])
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert np.isfinite(float(tr.last_kl)) and float(tr.last_kl) > 0 and tr.last_abs_sums.shape == (cfg.out_channels,)
    full = tr.full_state_dict()
    assert set(full) == set(sd)
    for k, v in before.items():
        assert torch.equal(sd[k], v), k                                         # nothing the caller passed in was written
    moved = [k for k in full if k.endswith(".weight") and not torch.equal(full[k], before[k])]
    assert any(k.startswith("encoder.") for k in moved) and any(k.startswith("decoder.") for k in moved)
    assert all(not torch.equal(full[k], before[k]) for k in full if k.startswith("encoder.") and k.endswith("conv.weight"))
    # sample_posterior=False: z = mean, and a drawn noise (generator) runs too
    assert np.isfinite(tr.train_step(images.cuda(), sample_posterior=False, as_float=True))
    assert np.isfinite(tr.train_step(images.cuda(), generator=torch.Generator().manual_seed(1), as_float=True))


# ---- hand-over ----------------------------------------------------------------------------------------------------------------------
def test_trained_vae_reaches_the_inference_vae(tmp_path):
    from rangeldm_amd.vae import AutoencoderKLHIP
    from rangeldm_amd.vae_training import VAETrainer
    o = oracle_step("TALL")
    cfg, images = o["cfg"], o["images"]
    vae = AutoencoderKLHIP(cfg)
    vae.load_state_dict(o["sd"])
    before = vae.encode(images.cuda()).latent_dist.parameters.cpu()
    tr = VAETrainer(cfg, o["sd"], lr=1e-3)
    for _ in range(2):
        loss = tr.train_step(images.cuda(), noise=o["noise"].cuda())
    assert np.isfinite(float(loss))
    trained = tr.full_state_dict()
    tr.save_pretrained(str(tmp_path))
    loaded = AutoencoderKLHIP.from_pretrained(str(tmp_path), subfolder="vae")
    again = loaded.state_dict()
    assert set(again) == set(trained)
    for k, v in trained.items():
        assert torch.equal(again[k], v.float()), k
    after = loaded.encode(images.cuda()).latent_dist.parameters.cpu()
    ref = o_vae.vae_encode(trained, cfg, images)
    tr.forward(images.cuda())
    err, err_tr = rel_l2(after, ref), rel_l2(tr.moments().cpu(), ref)
    print(f"encode with the trained weights: rel-L2 {err:.3g} against the oracle (the trainer's own moments {err_tr:.3g}), "
          f"{rel_l2(after, before):.3g} from the untrained encode")
    assert err < TOL_DECODE and err_tr < TOL_FWD
    assert rel_l2(after, before) > 1e-3
    tr.load_into(vae)                                                           # (the same weights on the same kernels)
    assert rel_l2(vae.encode(images.cuda()).latent_dist.parameters.cpu(), after) < 1e-3


def test_saved_state_continues_bit_identically(tmp_path):
    from rangeldm_amd.vae_training import VAETrainer
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    images, noise = _fixed_batch(cfg, 3, 9)
    a = VAETrainer(cfg, sd, lr=1e-3, deterministic=True)
    for _ in range(2):
        a.train_step(images.cuda(), noise=noise.cuda())
    path = str(tmp_path / "state.pt")
    a.save_state(path)
    for _ in range(2):
        a.train_step(images.cuda(), noise=noise.cuda())
    b = VAETrainer(cfg, sd, lr=1e-3, deterministic=True)
    b.load_state(path)
    assert b.global_step == 2
    losses = [float(b.train_step(images.cuda(), noise=noise.cuda())) for _ in range(2)]
    assert a.global_step == b.global_step == 4 and all(np.isfinite(v) for v in losses)
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x, y)


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_command_line_trains_everything_or_the_decoder(tmp_path, capsys):
    """--trainable all prints "kl" and moves encoder and decoder; --trainable decoder on the same seed prints lines without it and
    leaves the encoder alone."""
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.vae import AutoencoderKLHIP
    from rangeldm_amd.vae_training import save_vae_dir
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    src, inp = tmp_path / "src", tmp_path / "in"
    save_vae_dir(str(src), cfg, sd)
    inp.mkdir()
    g = torch.Generator().manual_seed(12)
    for i in range(3):
        np.save(str(inp / f"{i}.npy"), torch.rand(cfg.in_channels, *cfg.sample_size, generator=g).numpy())
    common = ["--weights", str(src), "--input", str(inp), "--steps", "3", "--batch-size", "2", "--lr", "1e-3", "--log-every", "2",
              "--seed", "4"]
    pixels = cfg.sample_size[0] * cfg.sample_size[1]
    for trainable, keys in (("all", {"step", "loss", "mae", "kl"}), ("decoder", {"step", "loss", "mae"})):
        out = tmp_path / trainable
        last = CLI.main(common + ["--out", str(out), "--trainable", trainable, "--kl-weight", "0.5"])
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert [l["step"] for l in lines] == [2, 3] and lines[-1] == last
        for l in lines:
            assert set(l) == keys
            rec = (WC[0] * l["mae"][0] + WC[1] * l["mae"][1]) * pixels
            kl = 0.5 * l["kl"] if trainable == "all" else 0.0
            assert np.isfinite(l["loss"]) and abs(l["loss"] - (rec + kl)) <= 1e-9 * l["loss"]
            assert trainable == "decoder" or l["kl"] > 0
        got = AutoencoderKLHIP.from_pretrained(str(out), subfolder="vae").state_dict()
        assert set(got) == set(sd)
        for k, v in sd.items():
            if k.endswith("conv.weight") or k.endswith("conv1.weight"):
                same = torch.equal(got[k], torch.from_numpy(v))
                assert same == (trainable == "decoder" and k.startswith("encoder.")), (trainable, k)
