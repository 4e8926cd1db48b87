"""GPU: decoder guidance (rangeldm_amd/guidance.py, csrc/guide.hip) -- the three kernels bit for bit against their numpy statements,
the tape's input-gradient-only replay against the full replay, DecoderGuide against fp64 autograd through the oracle decoder, and
LDMPipelineRange(decoder_guidance=) against the unguided eager loop, against itself and against the host statement of the whole loop.

The gradient gates are the project's rule for the VAE gradients: relative L2 to the fp64 statement at most TWICE the distance of the
bf16-operand host emulation from fp64, computed in the test (the tape's convs round their operands to bf16; nothing else separates them
from fp32).  Measured on an MI355X (device distance / gate):
    loss_and_grad            S: g_z 6.10e-03 / 1.21e-02, xhat 4.70e-03 / 9.46e-03      T: g_z 7.42e-03 / 1.53e-02, xhat 6.54e-03 / 1.31e-02
    refine, 3 iterations, against the bf16 statement
                             S: delta 4.59e-03 / 1.20e-02, L 2.64e-04 / 1.33e-03       T: delta 4.82e-03 / 1.54e-02, L 2.50e-04 / 1.07e-03
    10 guided steps on T, final latents against the fp64 loop: 5.05e-05 / 1.03e-04 (the guidance moved them by 7.82e-04)

The clause "fewer launches are issued than by the full replay" of the replay test is not counted with a profile counter: the library's
counters (rldm_unet_num_launches, rldm_sampler_profile) cover the inference plans, none covers the training tape.  The test counts the
weight-gradient calls the tape makes instead: none in the input-only replay, one per conv in the full one."""
import json

import numpy as np
import pytest
import torch

from oracle import schedulers as o_sched
from rangeldm_amd import guidance as G
from rangeldm_amd import train_ops as T
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP
from rangeldm_amd.synth import normal
from tests import guidance_util as U

pytestmark = pytest.mark.gpu
f32 = np.float32
PAIRS = (("beam4", "beam2"), ("span", "all"), ("none", "beam4"))          # every mask, a different one per image


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda().contiguous()


def same_bits(got, want):
    return U.bits(got).tobytes() == U.bits(want).tobytes()


_MODELS = {}


def models(name):
    """(AutoencoderKLHIP, its state dict, a deterministic DecoderGuide) of configuration `name`, built once."""
    from rangeldm_amd.vae import AutoencoderKLHIP
    if name not in _MODELS:
        sd = U.vae_weights(name)
        vae = AutoencoderKLHIP(U.CONFIGS[name])
        vae.load_state_dict(sd)
        _MODELS[name] = (vae, sd, G.DecoderGuide(vae, U.WC, deterministic=True))
    return _MODELS[name]


def pipeline(name="T"):
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.unet import UNet2DModelHIP
    key = "pipe/" + name
    if key not in _MODELS:
        unet = UNet2DModelHIP(U.UNET)
        unet.load_state_dict(U.unet_weights())
        _MODELS[key] = LDMPipelineRange(vae=models(name)[0], unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    return _MODELS[key]


# ---- the kernels, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("kind", ("integers", "random"))
@pytest.mark.parametrize("W,H", ((5, 3), (64, 16), (37, 7)))
def test_residual_matches_its_statement(W, H, kind, pair):
    B, C = 2, 2
    if kind == "integers":
        x = np.round(4 * normal(11, "dgg/x", (B, W, H, C))).astype(f32)
        y = np.round(4 * normal(11, "dgg/y", (B, C, W, H))).astype(f32)
    else:
        x, y = normal(12, "dgg/x", (B, W, H, C)), normal(12, "dgg/y", (B, C, W, H))
    m = U.mask_pair(*pair, W, H).numpy()
    wc = np.asarray(U.WC, f32)
    want_g, want_L = G.residual_host(x, y, m, wc)
    gx, L = T.guide_residual(dev(x), dev(y), dev(m), dev(wc))
    gx2, L2 = T.guide_residual(dev(x), dev(y), dev(m), dev(wc))
    assert same_bits(gx, want_g)
    got_L = L.cpu().numpy()
    print(f"{W}x{H} {kind} {pair}: L {got_L.tolist()} statement {want_L.tolist()}")
    assert np.all(np.abs(got_L - want_L) <= 1e-12 * np.abs(want_L))
    assert same_bits(L2, L) and same_bits(gx2, gx)                    # the same bits on every call
    for b, k in enumerate(pair):
        if k == "none":                                               # nothing known: L = 0 and g = +0
            assert got_L[b] == 0.0 and not U.bits(gx[b]).any()
        else:
            assert got_L[b] > 0.0
    # ... and at every batch position: image 0 alone, and twice in one batch
    x2, y2, m2 = np.stack([x[0], x[0]]), np.stack([y[0], y[0]]), np.stack([m[0], m[0]])
    _, Lr = T.guide_residual(dev(x2), dev(y2), dev(m2), dev(wc))
    _, L1 = T.guide_residual(dev(x[:1]), dev(y[:1]), dev(m[:1]), dev(wc))
    assert same_bits(Lr[0], L[0]) and same_bits(Lr[1], L[0]) and same_bits(L1[0], L[0])
    # the deterministic switch changes nothing: the order is fixed either way
    prev = T.deterministic_enabled()
    T.deterministic(not prev)
    try:
        gx3, L3 = T.guide_residual(dev(x), dev(y), dev(m), dev(wc))
    finally:
        T.deterministic(prev)
    assert same_bits(L3, L) and same_bits(gx3, gx)


@pytest.mark.parametrize("shape", ((2, 4, 5, 3), (2, 4, 32, 8), (3, 1, 7, 37)))
def test_update_latent_and_correct_match_their_statements(shape):
    B, C, W, H = shape
    g = normal(13, "dgg/g", (B, W, H, C))
    z0, delta = normal(13, "dgg/z0", shape), normal(13, "dgg/delta", shape)
    z0.reshape(-1)[:2] = (-0.0, 0.0)
    inv_sf = G.inverse_scale(0.18215)
    assert same_bits(T.guide_latent(dev(z0), inv_sf), G.latent_host(z0, inv_sf))
    Ls = np.array([2.5, 0.0, 1e-20][:B])                              # image 1 (and 2) on the 1e-8 floor
    cases = [(Ls, 0.75, delta), (Ls, 0.0, np.zeros_like(delta)), (None, 3.0, np.zeros_like(delta)), (Ls * 0 + 7.0, 1.0, np.zeros_like(delta))]
    for L, scale, d0 in cases:
        zd, dd = dev(z0.copy()), dev(d0.copy())
        T.guide_update(dev(g), None if L is None else dev(L), scale, inv_sf, zd, dd)
        want_z, want_d = G.update_host(g, L, scale, inv_sf, z0, d0)
        assert same_bits(zd, want_z) and same_bits(dd, want_d)
        if scale == 0.0:                                              # z0 keeps its value, delta stays +0
            assert np.array_equal(zd.cpu().numpy(), z0) and not U.bits(dd).any()
    for c in (0.37, 1.0, float(f32(0.9991))):                         # (1: the last step's coefficient)
        assert same_bits(T.guide_correct(dev(z0), dev(delta), c), G.correct_host(z0, delta, c))
        for zero in (np.zeros_like(z0), -np.zeros_like(z0)):          # delta = 0: the bits of z_plain, its -0 included
            assert same_bits(T.guide_correct(dev(z0), dev(zero), c), z0)
    assert same_bits(T.guide_correct(dev(z0), dev(np.zeros_like(z0)), -0.37), z0)


# ---- the tape ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S", "T"))
def test_input_only_replay_is_the_full_replay_without_parameter_gradients(name, monkeypatch):
    vae, sd, guide = models(name)
    assert guide.deterministic and guide.exp_avg is None and guide.exp_avg_sq is None
    W, H = U.CONFIGS[name].sample_size
    z = dev(U.latent(21, 2))
    gx = dev(normal(21, "dgg/gx", (2, W, H, 2)))
    calls = []
    real = T.wgrad_bias
    monkeypatch.setattr(T, "wgrad_bias", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    guide.grads.zero_()
    guide.forward(z)
    g_only = guide.input_gradient(gx).clone()
    n_only = len(calls)
    assert n_only == 0 and not guide.grads.any()                     # no weight gradient ran, the flat buffer is untouched
    assert not T.wgrad_group_pending() and not T.reduce_pending()
    guide.forward(z)
    g_full = guide.input_gradient(gx, params=True)
    convs = sum(1 for n in guide.names if n.endswith(".weight") and len(guide.shapes[n]) == 4)
    assert len(calls) == convs and guide.grads.any()
    guide.grads.zero_()
    assert tuple(g_only.shape) == (2, 32, 8, 4) and torch.isfinite(g_only).all() and g_only.any()
    assert same_bits(g_only, g_full)
    # the input-only replay again: the same bits (deterministic mode), and the trainers' switch is back where it was
    guide.forward(z)
    assert same_bits(guide.input_gradient(gx), g_only) and not guide.grads.any()
    assert guide._params_on and not guide._dy_shared


def _fp64_and_floor(name, z, y, m):
    """-> ((L, g_z) in fp64, (L, g_z) with bf16 conv operands) of the host statement."""
    _, sd, _ = models(name)
    ref = G.loss_and_grad_host(sd, U.CONFIGS[name], z, y, m, U.WC)
    emu = G.loss_and_grad_host(sd, U.CONFIGS[name], z, y, m, U.WC, dtype=torch.float32, bf16_operands=True)
    return ref, emu


@pytest.mark.parametrize("name", ("S", "T"))
def test_loss_and_grad_against_fp64_autograd(name):
    from oracle import vae as o_vae
    vae, sd, guide = models(name)
    cfg = U.CONFIGS[name]
    W, H = cfg.sample_size
    z, y, m = U.latent(22, 2), U.known_image(22, 2, W, H), U.mask_pair("beam4", "span", W, H)
    (L64, g64), (Lb, gb) = _fp64_and_floor(name, z, y, m)
    yd, md = guide.prepare(y, m, 2)
    L, g = guide.loss_and_grad(dev(z), yd, md)
    assert L.dtype == torch.float64 and tuple(L.shape) == (2,) and tuple(g.shape) == (2, *U.LATENT) and not guide.grads.any()
    gate, err = 2 * U.rel_l2(gb, g64), U.rel_l2(g, g64)
    print(f"{name}: g_z rel-L2 to fp64 {err:.3e}, gate (2 x bf16-operand floor) {gate:.3e}")
    assert err <= gate
    # the loss: the reconstruction under the same gate, and the sum exactly that of the device's own reconstruction
    dec = {k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("decoder.")}
    x64 = o_vae.vae_decode(dec, cfg, z.double() / cfg.scaling_factor)
    with G.bf16_operand_convs():
        xb = o_vae.vae_decode({k: v.float() for k, v in dec.items()}, cfg, z / cfg.scaling_factor)
    xhat = T.unpack_output(guide.forward(dev(z))).cpu()
    gate_x, err_x = 2 * U.rel_l2(xb, x64), U.rel_l2(xhat, x64)
    print(f"{name}: xhat rel-L2 to fp64 {err_x:.3e}, gate {gate_x:.3e}; L {L.tolist()} fp64 {L64.tolist()} bf16 operands {Lb.tolist()}")
    assert err_x <= gate_x
    wc = torch.tensor(U.WC, dtype=torch.float64).view(1, 2, 1, 1)
    own = (m.double() * wc * (xhat - y).double() ** 2).sum((1, 2, 3))       # (the kernel's d is the fp32 difference)
    assert bool(((L.cpu() - own).abs() <= 1e-12 * own).all())
    # each image's result is its own: the images swapped give the swapped results, bit for bit
    L2, g2 = guide.loss_and_grad(dev(z.flip(0)), yd.flip(0).contiguous(), md.flip(0).contiguous())
    assert same_bits(L2.flip(0), L) and same_bits(g2.flip(0), g)


@pytest.mark.parametrize("name", ("S", "T"))
def test_refine_three_iterations_against_the_host_statement(name):
    vae, sd, guide = models(name)
    cfg = U.CONFIGS[name]
    W, H = cfg.sample_size
    z, y, m = U.latent(23, 2), U.known_image(23, 2, W, H), U.mask_pair("beam4", "beam2", W, H)
    z64, d64, L64 = G.refine_host(sd, cfg, z, y, m, 1.0, 3, channel_weights=U.WC)
    zb, db, Lb = G.refine_host(sd, cfg, z, y, m, 1.0, 3, channel_weights=U.WC, dtype=torch.float32, bf16_operands=True)
    yd, md = guide.prepare(y, m, 2)
    zin = dev(z)
    keep = zin.clone()
    zr, delta, L = guide.refine(zin, yd, md, 1.0, 3)
    assert same_bits(zin, keep) and tuple(L.shape) == (3, 2) and L.dtype == torch.float64
    gate_d, err_d = 2 * U.rel_l2(db, d64), U.rel_l2(delta, db)
    gate_L, err_L = 2 * U.rel_l2(Lb, L64), U.rel_l2(L, Lb)
    print(f"{name}: refine x3  delta rel-L2 to the bf16 statement {err_d:.3e} gate {gate_d:.3e}; L {err_L:.3e} gate {gate_L:.3e}; "
          f"L per iteration {L.tolist()}")
    assert err_d <= gate_d and err_L <= gate_L
    assert U.rel_l2(zr, zb) <= 2 * U.rel_l2(zb, z64)
    # delta is the sum of the updates: z0' = z0 - delta up to the roundings of three subtractions
    assert float((zin - delta - zr).abs().max()) <= 4 * 2 ** -24 * float(zin.abs().max() + delta.abs().max())
    _, _, Ls = guide.refine(zin, yd, md, 1e-3, 2)                     # a short step is a descent step: the measured loss goes down
    assert bool((Ls[1] < Ls[0]).all())
    z0, d0, L0 = guide.refine(zin, yd, md, 1.0, 0)
    assert same_bits(z0, zin) and not d0.any() and tuple(L0.shape) == (0, 2)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
def unguided_loop(pipe, x_T, steps):
    """The fused=False loop of LDMPipelineRange, spelled out: -> (final latents, the latents after every step)."""
    sch = pipe.scheduler
    sch.set_timesteps(steps)
    z = x_T.cuda().float() * sch.init_noise_sigma
    pe = torch.zeros((z.shape[0], 1, z.shape[2], z.shape[3]), device="cuda")
    pe[:, :, 0, :] = 1
    trace = []
    for t in sch.timesteps:
        eps = pipe.unet(torch.cat([sch.scale_model_input(z, t), pe], 1), t).sample
        z = sch.step(eps, t, z, eta=0.0).prev_sample
        trace.append(z)
    return z, trace


@pytest.mark.parametrize("pair", PAIRS)
def test_scale_zero_is_the_unguided_eager_loop_and_known_pixels_return(pair):
    pipe, (vae, _, guide) = pipeline(), models("T")
    W, H = U.TT.sample_size
    x_T, y, m = U.latent(31, 2, "xT"), U.known_image(31, 2, W, H), U.mask_pair(*pair, W, H)
    kw = dict(batch_size=2, num_inference_steps=4, latents=x_T, known=y, known_mask=m, decoder_guidance=guide, return_latents=True)
    img0, lat0, L0 = pipe(guidance_scale=0.0, **kw)
    want, _ = unguided_loop(pipe, x_T, 4)
    assert same_bits(lat0, want)
    plain = pipe(batch_size=2, num_inference_steps=4, latents=x_T, fused=False)
    known = (m > 0.5).expand(2, 2, W, H).cuda()
    assert same_bits(img0[~known], plain[~known]) and same_bits(img0[known], y.cuda()[known])
    assert tuple(L0.shape) == (2,) and L0.dtype == torch.float64
    # guided: the known pixels come back bit for bit, the rest moves (where anything is known)
    img1, lat1, L1 = pipe(guidance_scale=1.0, guidance_iters=2, **kw)
    assert torch.isfinite(img1).all() and same_bits(img1[known], y.cuda()[known])
    for b, k in enumerate(pair):
        assert same_bits(lat1[b], lat0[b]) == (k == "none"), (b, k)
    out = pipe(guidance_scale=1.0, batch_size=2, num_inference_steps=4, latents=x_T, known=y, known_mask=m, decoder_guidance=guide)
    assert tuple(out.shape) == (2, 2, W, H)


def test_seeded_calls_repeat_and_a_sample_does_not_depend_on_the_batch():
    """What the sampler computes for a sample -- its final latents and the loss it measured -- has the same bits alone (B = 1, at its
    sample_offset) and in a batch of two.  The decoded image is rldm_vae_decode's, whose conv routes depend on the batch size (its
    activations are bf16: alone and in a batch of two, single pixels were seen to differ by 2e-4; printed below), and at guidance_scale = 0 the image must
    equal the unguided call's at the same batch size; so the image is held to exactly that: the inference decode of those latents at
    the call's batch size with the known pixels pasted over it."""
    from rangeldm_amd.rng import DeviceGenerator
    pipe, (vae, _, guide) = pipeline(), models("T")
    sf = vae.config.scaling_factor
    W, H = U.TT.sample_size
    y, m = U.known_image(32, 2, W, H), U.mask_pair("beam4", "span", W, H)
    kw = dict(num_inference_steps=4, decoder_guidance=guide, guidance_scale=1.0, return_latents=True)
    a = pipe(batch_size=2, generator=DeviceGenerator(77), known=y, known_mask=m, **kw)
    b = pipe(batch_size=2, generator=DeviceGenerator(77), known=y, known_mask=m, **kw)
    assert all(same_bits(p, q) for p, q in zip(a, b))
    c = pipe(batch_size=2, generator=DeviceGenerator(78), known=y, known_mask=m, **kw)
    assert not same_bits(c[1], a[1])
    for i in range(2):                                                # sample i alone, at its own offset
        one = pipe(batch_size=1, generator=DeviceGenerator(77), sample_offset=i, known=y[i:i + 1], known_mask=m[i:i + 1], **kw)
        assert same_bits(one[1][0], a[1][i]) and same_bits(one[2][0], a[2][i])
        known = (m[i:i + 1] > 0.5).expand(1, 2, W, H).cuda()
        assert same_bits(one[0], torch.where(known, y[i:i + 1].cuda(), vae.decode(one[1] / sf).sample))
        print(f"sample {i}: image alone against in a batch of two, max |difference| {float((one[0][0] - a[0][i]).abs().max()):.3e} "
              f"(the inference decode's own: {float((vae.decode(a[1][i:i + 1] / sf).sample[0] - vae.decode(a[1] / sf).sample[i]).abs().max()):.3e})")
    assert same_bits(a[0], torch.where((m > 0.5).expand(2, 2, W, H).cuda(), y.cuda(), vae.decode(a[1] / sf).sample))


def test_window_leaves_the_first_half_unguided():
    pipe, (vae, _, guide) = pipeline(), models("T")
    W, H = U.TT.sample_size
    x_T, y, m = U.latent(33, 2, "xT"), U.known_image(33, 2, W, H), U.mask_pair("beam4", "beam2", W, H)
    trace = []
    pipe(batch_size=2, num_inference_steps=6, latents=x_T, known=y, known_mask=m, decoder_guidance=guide, guidance_start=0.5,
         guidance_stop=1.0, latent_trace=trace)
    _, want = unguided_loop(pipe, x_T, 6)
    assert len(trace) == 6
    assert all(same_bits(trace[i], want[i]) for i in range(3)) and not any(same_bits(trace[i], want[i]) for i in range(3, 6))


def test_ten_guided_steps_against_the_host_statement():
    """T, 10 steps, scale 1, one iteration per step: the final latents against decoder_guided_sample_host in fp64, gated by twice the
    distance of its bf16-operand form from fp64.  All three loops ask the SAME network for eps (the HIP UNet), so what is compared is the
    guidance and the scheduler, not the UNet's own bf16 error."""
    pipe, (vae, sd, guide) = pipeline(), models("T")
    W, H = U.TT.sample_size
    x_T, y, m = U.latent(34, 2, "xT"), U.known_image(34, 2, W, H), U.mask_pair("beam4", "span", W, H)
    unet = lambda x, t: pipe.unet(x.float().cuda(), t).sample.cpu()          # noqa: E731
    args = (sd, U.TT, x_T, y, m, 10)
    lat64, L64 = G.decoder_guided_sample_host(unet, o_sched.OracleDDIMScheduler(), *args, channel_weights=U.WC, pos_encoding=True)
    latb, Lb = G.decoder_guided_sample_host(unet, o_sched.OracleDDIMScheduler(), *args, channel_weights=U.WC, pos_encoding=True,
                                            dtype=torch.float32, bf16_operands=True)
    plain, _ = unguided_loop(pipe, x_T, 10)
    _, lat, L = pipe(batch_size=2, num_inference_steps=10, latents=x_T, known=y, known_mask=m, decoder_guidance=guide,
                     return_latents=True)
    gate, err = 2 * U.rel_l2(latb, lat64), U.rel_l2(lat, lat64)
    print(f"10 guided steps: final latents rel-L2 to fp64 {err:.3e}, gate {gate:.3e}; guidance moved them by {U.rel_l2(plain, lat64):.3e}; "
          f"last L {L.tolist()} fp64 {L64.tolist()}")
    assert err <= gate
    assert U.rel_l2(plain, lat64) > gate                              # (the guidance is what is being measured)


def test_refusals_on_the_device():
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.vae import AutoencoderKLHIP
    pipe, (vae, sd, guide) = pipeline(), models("T")
    W, H = U.TT.sample_size
    y, m = U.known_image(35, 1, W, H), U.mask_pair("beam4", "beam4", W, H)[:1]
    with pytest.raises(ValueError, match="pixel-space"):              # without the argument: what it raised before
        pipe(batch_size=1, num_inference_steps=2, known=y, known_mask=m)
    kw = dict(batch_size=1, num_inference_steps=2, known=y, known_mask=m, decoder_guidance=guide)
    for sch in (DDPMSchedulerHIP(), DPMSolverMultistepSchedulerHIP()):
        other = LDMPipelineRange(vae=vae, unet=pipe.unet, scheduler=sch, pos_encoding=True)
        with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
            other(**kw)
    for bad in (dict(eta=0.3), dict(jump_length=2), dict(jump_n_sample=2), dict(final_only=False)):
        with pytest.raises(NotImplementedError):
            pipe(**kw, **bad)
    with pytest.raises(ValueError, match="known"):
        pipe(batch_size=1, num_inference_steps=2, decoder_guidance=guide)
    with pytest.raises(TypeError):
        pipe(**dict(kw, decoder_guidance="yes"))
    # decoder_guidance=True builds one guide and keeps it; a reloaded VAE makes a guide stale
    v2 = AutoencoderKLHIP(U.TT)
    v2.load_state_dict(sd)
    p2 = LDMPipelineRange(vae=v2, unet=pipe.unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    with pytest.raises(ValueError, match="another VAE"):
        p2(**kw)
    x_T = U.latent(35, 1, "xT")
    a = p2(**dict(kw, decoder_guidance=True, latents=x_T))
    first = p2._guide
    assert not first.stale(v2) and first.stale(vae)
    b = p2(**dict(kw, decoder_guidance=True, latents=x_T))            # (that guide is not in the deterministic mode: no bits promised)
    assert p2._guide is first and torch.isfinite(a).all() and torch.isfinite(b).all()
    v2.load_state_dict(sd)
    assert first.stale(v2)
    p2(**dict(kw, decoder_guidance=True, latents=x_T))
    assert p2._guide is not first and not p2._guide.stale(v2)


def test_driver_densifies_with_the_latent_model_and_evaluate_reads_it(tmp_path):
    from rangeldm_amd import evaluate, inference_conditional
    out = tmp_path / "dg"
    inference_conditional.main(["--guided", "--task", "densification", "--cfg", "RangeLDM", "--decoder-guidance", "--guidance-scale", "0.5",
                                "--guidance-iters", "1", "--guidance-window", "0", "1", "--samples", "1", "--batch_size", "2", "--steps", "2",
                                "--save-npy", "--out", str(out)])
    for d in ("densification_result", "densification_target", "densification_input"):
        assert sorted(p.name for p in (out / d).iterdir())[:3] == ["0_seed_0.bin", "0_seed_0.npy", "0_seed_0.png"]
    res = np.load(out / "densification_result" / "1_seed_0.npy")
    tgt = np.load(out / "densification_target" / "1_seed_0.npy")
    assert res.shape == (2, 1024, 64) and np.isfinite(res).all()
    assert np.array_equal(res[..., 2::4], tgt[..., 2::4]) and not np.array_equal(res, tgt)
    r = evaluate.main(["densification", "--exp", str(out), "--json", str(tmp_path / "d.json")])
    assert r["task"] == "densification" and r["pairs"] == 2 and r["rate"] == 4
    assert json.loads((tmp_path / "d.json").read_text())["pairs"] == 2
    assert all(np.isfinite(v) for v in r["mae_m"].values())
