"""CPU: the host statements of decoder guidance (rangeldm_amd/guidance.py) -- the numpy restatements of csrc/guide.hip against literal
loops over the elements, the correction's zero case, the algebra of c_i, the whole-loop statement at scale 0 against the oracle's DDIM
loop, its fp64 gradient against finite differences of sqrt(L), and the refusals."""
import math

import numpy as np
import pytest
import torch

from oracle import schedulers as o_sched, unet as o_unet, vae as o_vae
from rangeldm_amd import guidance as G
from rangeldm_amd.config import SchedulerConfig
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP
from rangeldm_amd.synth import normal
from tests import guidance_util as U

f32 = np.float32


def _operands(seed, B=2, C=2, W=5, H=3):
    x = normal(seed, "dgh/x", (B, W, H, C))
    y = normal(seed, "dgh/y", (B, C, W, H))
    m = (normal(seed, "dgh/m", (B, 1, W, H)) > 0).astype(f32)
    return x, y, m


def test_residual_statement_is_the_literal_loop():
    x, y, m = _operands(1)
    wc = np.asarray(U.WC, f32)
    gx, L = G.residual_host(x, y, m, wc)
    B, W, H, C = x.shape
    assert gx.dtype == f32 and L.dtype == np.float64
    for b in range(B):
        terms = []
        for w in range(W):
            for h in range(H):
                for c in range(C):
                    d = f32(x[b, w, h, c] - y[b, c, w, h])
                    if m[b, 0, w, h] > 0.5:
                        want = f32(f32(f32(2.0) * wc[c]) * d)
                        terms.append(float(wc[c]) * float(d) * float(d))
                    else:
                        want = f32(0.0)
                        terms.append(0.0)
                    assert gx[b, w, h, c].tobytes() == want.tobytes()
        # 30 elements: one partial; the statement's tree is a sum of the same terms, equal to math.fsum to the last bits
        assert abs(L[b] - math.fsum(terms)) <= 1e-15 * abs(L[b])
    # the order of the sum is fixed per image: the same image at another batch position gives the same bits
    _, L2 = G.residual_host(x[::-1], y[::-1], m[::-1], wc)
    assert L2[::-1].tobytes() == L.tobytes()
    # more than one partial (2 * 40 * 7 = 560 elements per image: three partials of 256 lanes, the last one short)
    x, y, m = _operands(2, W=40, H=7)
    _, L = G.residual_host(x, y, m, wc)
    d = (x - y.transpose(0, 2, 3, 1)).astype(np.float64)
    want = (np.broadcast_to(m.transpose(0, 2, 3, 1), d.shape) * wc.astype(np.float64) * d * d).sum((1, 2, 3))
    assert np.allclose(L, want, rtol=1e-13, atol=0)


def test_update_and_latent_statements_are_the_literal_loops():
    B, C, W, H = 2, 4, 5, 3
    g = normal(3, "dgh/g", (B, W, H, C))
    z0, delta = normal(3, "dgh/z0", (B, C, W, H)), normal(3, "dgh/delta", (B, C, W, H))
    L = np.array([2.5, 0.0])                                      # the second image sits on the 1e-8 floor
    inv_sf, scale = G.inverse_scale(0.18215), 0.75
    zn, dn = G.update_host(g, L, scale, inv_sf, z0, delta)
    zin = G.latent_host(z0, inv_sf)
    for b in range(B):
        rho = f32(scale / max(math.sqrt(L[b]), 1e-8))
        for c in range(C):
            for w in range(W):
                for h in range(H):
                    u = f32(rho * f32(g[b, w, h, c] * f32(inv_sf)))
                    assert zn[b, c, w, h].tobytes() == f32(z0[b, c, w, h] - u).tobytes()
                    assert dn[b, c, w, h].tobytes() == f32(delta[b, c, w, h] + u).tobytes()
                    assert zin[b, w, h, c].tobytes() == f32(z0[b, c, w, h] * f32(inv_sf)).tobytes()
    assert float(np.float32(0.75 / 1e-8)) == float(f32(scale / max(math.sqrt(L[1]), 1e-8)))
    # L None: rho = 1, so delta' - delta is the scaled gradient itself
    _, d1 = G.update_host(g, None, 123.0, inv_sf, z0, np.zeros_like(delta))
    assert d1.tobytes() == (g * f32(inv_sf)).transpose(0, 3, 1, 2).astype(f32).tobytes()
    # scale 0: z0 keeps its value and delta stays +0
    z2, d2 = G.update_host(g, L, 0.0, inv_sf, z0, np.zeros_like(delta))
    assert np.array_equal(z2, z0) and not np.signbit(d2).any() and not d2.any()


def test_correct_statement_and_its_zero_case():
    z = normal(4, "dgh/zp", (2, 4, 5, 3))
    z.reshape(-1)[:4] = (-0.0, 0.0, -0.0, 1.5)
    delta = normal(4, "dgh/d", z.shape)
    c = f32(0.37)
    got = G.correct_host(z, delta, c)
    for i, (a, d) in enumerate(zip(z.reshape(-1), delta.reshape(-1))):
        p = f32(c * d)
        assert got.reshape(-1)[i].tobytes() == (a if p == 0 else f32(a - p)).tobytes()
    for zero in (np.zeros_like(z), -np.zeros_like(z)):
        for cc in (c, f32(-0.37), f32(1.0)):
            assert G.correct_host(z, zero, cc).tobytes() == z.tobytes()          # -0.0 included


def test_coefficient_is_the_ddim_step_with_the_corrected_estimate():
    """z_plain - c_i delta == a_p (z0 - delta) + s_p (z_t - a_t (z0 - delta)) / s_t, for every timestep of a 10-step schedule, for both
    schedulers' alphas; 1 on the last step."""
    for sch in (o_sched.OracleDDIMScheduler(), DDIMSchedulerHIP()):
        sch.set_timesteps(10)
        g = torch.Generator().manual_seed(0)
        z_t, z0, delta = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
        for t in sch.timesteps:
            at, ap = G._alpha_pair(sch, t)
            a_t, s_t, a_p, s_p = math.sqrt(at), math.sqrt(1 - at), math.sqrt(ap), math.sqrt(1 - ap)
            plain = a_p * z0 + s_p * (z_t - a_t * z0) / s_t
            want = a_p * (z0 - delta) + s_p * (z_t - a_t * (z0 - delta)) / s_t
            c = G.guidance_coefficient(sch, t, rounded=False)
            assert (plain - c * delta - want).abs().max() < 1e-13
            assert abs(G.guidance_coefficient(sch, t) - c) <= 2 ** -24 * abs(c)
        assert G.guidance_coefficient(sch, sch.timesteps[-1]) == 1.0 and G.guidance_coefficient(sch, sch.timesteps[0]) > 0


def test_window():
    assert G.guided_steps(10) == list(range(10))
    assert G.guided_steps(10, 0.5, 1.0) == [5, 6, 7, 8, 9]
    assert G.guided_steps(7, 0.0, 0.5) == [0, 1, 2, 3]
    assert G.guided_steps(10, 0.3, 0.3) == []
    for bad in ((-0.1, 1.0), (0.6, 0.5), (0.0, 1.1)):
        with pytest.raises(ValueError, match="window"):
            G.guided_steps(10, *bad)


def _host_models():
    sd, usd = U.vae_weights("S"), U.unet_weights()
    ounet = o_unet.OracleUNet(U.UNET, usd)
    return sd, (lambda x, t: ounet(x.float(), t).sample)


def test_scale_zero_is_the_oracle_ddim_loop_exactly():
    sd, unet = _host_models()
    W, H = U.S.sample_size
    x_T, y, m = U.latent(5, 2), U.known_image(5, 2, W, H), U.mask_pair("beam4", "span", W, H)
    for dtype, bf in ((torch.float32, True), (torch.float64, False)):
        sch = o_sched.OracleDDIMScheduler()
        trace = []
        got, last = G.decoder_guided_sample_host(unet, sch, sd, U.S, x_T, y, m, 3, guidance_scale=0.0, guidance_iters=2, dtype=dtype,
                                                 bf16_operands=bf, pos_encoding=True, trace=trace)
        ref = o_sched.OracleDDIMScheduler()
        ref.set_timesteps(3)
        z = x_T.to(dtype)
        pe = torch.zeros((2, 1, 32, 8), dtype=dtype)
        pe[:, :, 0, :] = 1
        for i, t in enumerate(ref.timesteps):
            z = ref.step(unet(torch.cat([z, pe], 1), t).to(dtype), t, z).prev_sample
            assert torch.equal(trace[i], z)
        assert torch.equal(got, z) and got.dtype == dtype
        assert last is not None and bool((last > 0).all())           # the loss is still measured
    # no iterations, or an empty window: plain steps, nothing measured
    for kw in (dict(guidance_iters=0), dict(guidance_start=0.5, guidance_stop=0.5)):
        again, none = G.decoder_guided_sample_host(unet, o_sched.OracleDDIMScheduler(), sd, U.S, x_T, y, m, 3, guidance_scale=1.0,
                                                   pos_encoding=True, **kw)
        assert torch.equal(again, z) and none is None


def test_fp64_gradient_matches_finite_differences_of_sqrt_loss():
    """d sqrt(L_b) / d z0 = g_z / (2 sqrt(L_b)) against central differences along random directions and single coordinates, on S, in the
    fp64 statement: 1e-6 relative."""
    sd = U.vae_weights("S")
    W, H = U.S.sample_size
    z, y, m = U.latent(6, 2).double(), U.known_image(6, 2, W, H), U.mask_pair("beam4", "beam2", W, H)
    L, g = G.loss_and_grad_host(sd, U.S, z, y, m, U.WC)
    assert L.dtype == torch.float64 and bool((L > 0).all())
    gs = g / (2 * L.sqrt()).view(-1, 1, 1, 1)
    gen = torch.Generator().manual_seed(6)
    dirs = [torch.randn(z.shape, generator=gen, dtype=torch.float64) for _ in range(3)]
    for idx in ((0, 0, 0, 0), (1, 3, 31, 7), (0, 2, 16, 4)):
        e = torch.zeros_like(z)
        e[idx] = 1.0
        dirs.append(e + e.flip(0) if idx[0] == 0 else e)
    h = 1e-5
    for v in dirs:
        v = v / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1).clamp(min=1e-30)
        lp, _ = G.loss_and_grad_host(sd, U.S, z + h * v, y, m, U.WC)
        lm, _ = G.loss_and_grad_host(sd, U.S, z - h * v, y, m, U.WC)
        fd = (lp.sqrt() - lm.sqrt()) / (2 * h)
        an = (gs * v).flatten(1).sum(1)
        scale = gs.flatten(1).norm(dim=1)
        print(f"finite differences: {fd.tolist()} analytic {an.tolist()} (|grad| {scale.tolist()})")
        assert bool(((fd - an).abs() <= 1e-6 * scale).all())
    # an all-unknown mask measures nothing
    L0, g0 = G.loss_and_grad_host(sd, U.S, z, y, U.mask_pair("none", "none", W, H), U.WC)
    assert not L0.any() and not g0.any()


def test_bf16_operand_statement_is_close_to_fp64_and_restores_the_oracle():
    from oracle import ops as o_ops
    sd = U.vae_weights("S")
    W, H = U.S.sample_size
    z, y, m = U.latent(7, 2), U.known_image(7, 2, W, H), U.mask_pair("beam4", "span", W, H)
    plain = o_ops.circ_conv2d
    L64, g64 = G.loss_and_grad_host(sd, U.S, z, y, m, U.WC)
    Lb, gb = G.loss_and_grad_host(sd, U.S, z, y, m, U.WC, dtype=torch.float32, bf16_operands=True)
    assert o_ops.circ_conv2d is plain
    assert gb.dtype == torch.float32 and 1e-5 < U.rel_l2(gb, g64) < 5e-2 and U.rel_l2(Lb, L64) < 5e-2
    x64 = o_vae.vae_decode({k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("decoder.")}, U.S, z.double() / 0.18215)
    assert x64.dtype == torch.float64


def test_refusals():
    from rangeldm_amd.pipelines import LDMPipelineRange
    ok = DDIMSchedulerHIP()
    G.refuse_unsupported(ok, 0.0, 1, 1, True)
    for sch in (DDPMSchedulerHIP(), DPMSolverMultistepSchedulerHIP(SchedulerConfig())):
        with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
            G.refuse_unsupported(sch, 0.0, 1, 1, True)
    with pytest.raises(NotImplementedError, match="eta"):
        G.refuse_unsupported(ok, 0.5, 1, 1, True)
    for jl, jn in ((2, 1), (1, 2)):
        with pytest.raises(NotImplementedError, match="resample"):
            G.refuse_unsupported(ok, 0.0, jl, jn, True)
    with pytest.raises(NotImplementedError, match="final image"):
        G.refuse_unsupported(ok, 0.0, 1, 1, False)
    # the pipeline refuses before it touches a model or draws anything
    pipe = LDMPipelineRange(vae=None, unet=None, scheduler=DDPMSchedulerHIP())
    with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
        pipe(decoder_guidance=True, known=torch.zeros(1, 2, 8, 8), known_mask=torch.ones(1, 1, 8, 8))
    pipe = LDMPipelineRange(vae=None, unet=None, scheduler=ok)
    for kw in (dict(eta=0.1), dict(jump_length=2), dict(jump_n_sample=3), dict(final_only=False)):
        with pytest.raises(NotImplementedError):
            pipe(decoder_guidance=True, known=torch.zeros(1, 2, 8, 8), known_mask=torch.ones(1, 1, 8, 8), **kw)


def test_command_line_flags():
    from rangeldm_amd import inference_conditional as IC
    with pytest.raises(ValueError, match="pixel-space"):
        IC.main(["--guided", "--task", "densification", "--cfg", "RangeDM", "--decoder-guidance", "--samples", "1"])
    with pytest.raises(NotImplementedError, match="DDIM"):
        IC.main(["--guided", "--cfg", "RangeLDM", "--decoder-guidance", "--scheduler", "ddpm", "--samples", "1"])
    with pytest.raises(NotImplementedError, match="resample"):
        IC.main(["--guided", "--cfg", "RangeLDM", "--decoder-guidance", "--jump-length", "2", "--samples", "1"])
