"""GPU: UniPC -- rldm_sched_unipc_step against numpy at every size at which the kernel takes another path, the public step against
the restated scheduler through every order transition and on the Gaussian problem, the captured sampler (RLDM_SAMPLER_UNIPC: the
step as a launch of its own behind conv_out, `last` and the x0 history per lane) against the eager loop on every pipeline, the eager
loop against the oracle networks, the refusals and the sampling driver."""
import ctypes as C

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd.config import VAEConfig
from rangeldm_amd.schedulers import DDIMSchedulerHIP, UniPCMultistepSchedulerHIP, repaint_program
from rangeldm_amd.synth import normal
from oracle import pipelines as o_pipe, unet as o_unet, vae as o_vae
from tests.hip_util import rel_l2
from tests.test_dpmsolver_gpu import PTYPES, TOL_FWD, T, hip_unet, hip_vae, small_cfg
from tests.test_dpmsolver_host import exact_eps, ode_target
from tests.test_unipc_host import RestatedUniPC, apply_row, run_unipc

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one group short of a vector, tail only; 15 groups + tail; whole groups; groups + 1; several workgroups with two misaligned history
# slots; and more groups than the 2048 x 256 threads of the largest grid (the grid-stride loop), with a tail
SIZES = (1, 3, 63, 64, 65, 3001, 2048 * 256 * 4 + 1027)


def unipc(**kw):
    return UniPCMultistepSchedulerHIP(**kw)


# ---- the elementwise entry point ------------------------------------------------------------------------------------------
_ROWS = {}


def step_rows(ptype):
    """row 0 (no corrector), row 1 (UniC-1 + UniP-2) and row 4 (UniC-3 + UniP-3) of a ten-step order-3 schedule"""
    if ptype not in _ROWS:
        sch = unipc(prediction_type=ptype, solver_order=3)
        sch.set_timesteps(10)
        tab = sch.coefficients()
        assert tab[0, 2] == 0 and tab[1, 2] == 1 and tab[1, 10] != 0 and tab[1, 11] == 0 and tab[1, 5] == 0
        assert tab[4, 2] == 1 and tab[4, 6] != 0 and tab[4, 11] != 0
        _ROWS[ptype] = (sch.prediction_code, [(tab[0], 0), (tab[1], 1), (tab[4], 3)])
    return _ROWS[ptype]


def call_step(code, row, out, x, last, hist, x_prev, n):
    cf = (C.c_float * 12)(*[float(v) for v in row])
    p = _lib.ptr
    _lib.check(_lib.lib().rldm_sched_unipc_step(code, cf, p(out), p(x), p(last), p(hist), p(x_prev), n, _lib.stream_ptr(x.device)),
               "rldm_sched_unipc_step")
    torch.cuda.synchronize()


# (the grid-stride size runs once: the loop does not depend on the prediction type)
@pytest.mark.parametrize("ptype,n", [(p, n) for p in PTYPES for n in SIZES[:-1]] + [("epsilon", SIZES[-1])])
def test_sched_unipc_step_matches_numpy(ptype, n):
    """`filled` = how many history slots (and whether `last`) hold numbers; the rest is NaN, which a row that has no use for it must
    neither read into a result nor fail to shift."""
    code, rows = step_rows(ptype)
    rng = np.random.default_rng(n)
    out, x, last0, h0, h1, h2 = (rng.standard_normal(n).astype(np.float32) for _ in range(6))
    for row, filled in rows:
        last = last0 if filled >= 1 else np.full(n, np.nan, np.float32)
        hist = np.stack([h if k < filled else np.full(n, np.nan, np.float32) for k, h in enumerate((h0, h1, h2))])
        f64 = [a.astype(np.float64) for a in (out, x, last, *hist)]
        x_c, x_next, m = apply_row(row.astype(np.float64), ptype, f64[0], f64[1], f64[2], f64[3:])
        want = {"x_prev": x_next, "last": x_c, "hist0": m, "hist1": f64[3], "hist2": f64[4]}
        got_by_alias = []
        for alias in (False, True):
            d_out, d_x, d_last, d_hist = (T(a.copy()).to(DEV) for a in (out, x, last, hist))
            d_prev = d_x if alias else torch.full((n,), float("nan"), device=DEV)
            call_step(code, row, d_out, d_x, d_last, d_hist, d_prev, n)
            hh = d_hist.cpu().double().numpy()
            got = {"x_prev": d_prev.cpu().double().numpy(), "last": d_last.cpu().double().numpy(), "hist0": hh[0], "hist1": hh[1],
                   "hist2": hh[2]}
            if not alias:
                assert torch.equal(d_x.cpu(), T(x)) and torch.equal(d_out.cpu(), T(out))        # inputs untouched
            for k in ("x_prev", "last", "hist0"):
                assert np.isfinite(got[k]).all(), (k, filled)                                   # no NaN leaked
            for k, w in want.items():
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(got[k]), nan), (k, filled, alias)                # (a shifted empty slot stays empty)
                if not nan.all():
                    err = np.abs(got[k] - w)[~nan].max()
                    assert err < 2e-5 * (1 + np.abs(w[~nan]).max()), (k, filled, alias, err)
            got_by_alias.append(got)
        for k in want:
            assert np.array_equal(got_by_alias[0][k], got_by_alias[1][k], equal_nan=True), k    # x_prev aliasing x: the same bits


def test_sched_unipc_step_refuses_overlapping_state():
    n = 64
    buf = torch.zeros(6 * n, device=DEV)
    row = step_rows("epsilon")[1][0][0]
    out, x, last, hist = buf[:n], buf[n:2 * n], buf[2 * n:3 * n], buf[3 * n:]
    call_step(0, row, out, x, last, hist, x, n)
    for bad in (dict(last=x), dict(hist=buf[2 * n:5 * n]), dict(last=buf[4 * n:5 * n]), dict(hist=buf[:3 * n])):
        kw = dict(out=out, x=x, last=last, hist=hist)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="overlap"):
            call_step(0, row, kw["out"], kw["x"], kw["last"], kw["hist"], kw["x"], n)
    # x_prev: x itself (above) or a tensor of its own, never part of x or of the model output
    wide = torch.zeros(8 * n, device=DEV)
    o2, x2, l2, h2 = wide[:n], wide[2 * n:3 * n], wide[4 * n:5 * n], wide[5 * n:]
    call_step(0, row, o2, x2, l2, h2, wide[3 * n:4 * n], n)
    for bad_prev in (wide[2 * n + 4:3 * n + 4], wide[n // 2:n + n // 2]):
        with pytest.raises(RuntimeError, match="overlap"):
            call_step(0, row, o2, x2, l2, h2, bad_prev, n)


# ---- the public step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", PTYPES)
def test_public_step_matches_restatement_through_every_order(ptype):
    """Five steps at order 3 run with orders 1, 2, 3, 2, 1 (corrector orders 1, 2, 3, 2): the history shift and the `last` hand-over
    across each transition, both schedulers free-running on the same model outputs.  Bound: the entry point's 2e-5 (1 + max|want|) per
    step, and a step passes an earlier error on with |p_x|, |k_last| <= 1, so five of them."""
    shape = (2, 4, 32, 8)
    sch = unipc(prediction_type=ptype, solver_order=3)
    ref = RestatedUniPC(ptype, 3)
    x = normal(91, "unipc/x", shape)
    outs = [normal(91, f"unipc/out/{i}", shape) for i in range(5)]
    runs = []
    for _ in range(2):                                       # (twice: set_timesteps resets the state)
        sch.set_timesteps(5)
        assert sch.step_index is None
        ref.set_timesteps(5)
        xd, xr = T(x).to(DEV), T(x).double()
        for i, t in enumerate(sch.timesteps):
            xd = sch.step(T(outs[i]).to(DEV), t, xd).prev_sample
            xr = ref.advance(T(outs[i]).double(), xr)[1]
            assert sch.step_index == i + 1
            err = float((xd.cpu().double() - xr).abs().max())
            assert torch.isfinite(xd).all() and err < (i + 1) * 2e-5 * (1 + float(xr.abs().max())), (i, err)
        for got, want in ((sch._last, ref.last), *zip(sch._hist, ref.m)):
            assert float((got.cpu().double() - want).abs().max()) < 5 * 2e-5 * (1 + float(want.abs().max()))
        runs.append(xd.cpu())
    assert torch.equal(runs[0], runs[1])
    with pytest.raises(ValueError, match="more often"):
        sch.step(T(outs[0]).to(DEV), 0, xd)


def test_public_step_started_behind_the_first_timestep_warms_up_from_there():
    """diffusers' lower_order_nums counts steps, not indices: a run that starts at index 2 takes a first-order step without a corrector"""
    shape = (1, 4, 32, 8)
    sch = unipc(solver_order=3)
    sch.set_timesteps(6)
    ref = RestatedUniPC("epsilon", 3)
    ref.set_timesteps(6)
    ref.i = 2
    xd, xr = T(normal(92, "unipc/x", shape)).to(DEV), T(normal(92, "unipc/x", shape)).double()
    for i in range(2, 6):
        out = normal(92, f"unipc/out/{i}", shape)
        xd = sch.step(T(out).to(DEV), sch.timesteps[i], xd).prev_sample
        xr = ref.advance(T(out).double(), xr)[1]
        assert float((xd.cpu().double() - xr).abs().max()) < (i - 1) * 2e-5 * (1 + float(xr.abs().max())), i


@pytest.mark.parametrize("order", (2, 3))
@pytest.mark.parametrize("n", (10, 20))
def test_public_step_on_gaussian_data(n, order):
    """The device's fp32 trajectory ends as close to the exact ODE solution as the same rows run in float64 on the host, plus 1e-5."""
    sch = unipc(solver_order=order)
    sch.set_timesteps(n)
    rows = sch.coefficients()
    x_T = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    target = ode_target(x_T.astype(np.float64), float(rows[0, 0]), float(rows[0, 1]))
    host = float(np.abs(run_unipc(rows, x_T.astype(np.float64)) - target).max())
    x = T(x_T).to(DEV)
    for i, t in enumerate(sch.timesteps):
        eps = exact_eps(x.cpu().double().numpy(), float(rows[i, 0]), float(rows[i, 1]))
        x = sch.step(T(eps.astype(np.float32)).to(DEV), t, x).prev_sample
    dev = float(np.abs(x.cpu().double().numpy() - target).max())
    print(f"UniPC-{order}, {n} steps: device error {dev:.6e}, host float64 error {host:.6e}")
    assert dev <= host + 1e-5


# ---- pipelines ---------------------------------------------------------------------------------------------------------------
def ldm_pipe(sch, unet=None):
    from rangeldm_amd.pipelines import LDMPipelineRange
    unet = unet if unet is not None else hip_unet(small_cfg(5, 4), "dpm/small.")[0]
    return LDMPipelineRange(vae=hip_vae()[0], unet=unet, scheduler=sch, pos_encoding=True)


def test_eager_ldm_loop_matches_oracle():
    cfg = small_cfg(5, 4)
    unet, sd = hip_unet(cfg, "dpm/small.")
    _, vsd = hip_vae()
    x_T = T(normal(93, "unipc/xT", (2, 4, 32, 8)))
    img = ldm_pipe(unipc(solver_order=3), unet)(batch_size=2, num_inference_steps=8, latents=x_T, output_type="torch", fused=False).cpu()
    ref = o_pipe.ldm_pipeline(o_vae.OracleVAE(VAEConfig(), vsd), o_unet.OracleUNet(cfg, sd), RestatedUniPC("epsilon", 3), x_T, 8,
                              pos_encoding=True)
    e = rel_l2(img, ref)
    print(f"eager UniPC-3 8 steps vs oracle: rel-L2 {e:.3e}")
    assert torch.isfinite(img).all() and e < 3 * TOL_FWD


@pytest.mark.parametrize("ptype,order", [(p, 2) for p in PTYPES] + [("epsilon", 3), ("epsilon", 1)])
def test_captured_ldm_sampler_matches_eager_loop(ptype, order):
    x_T = T(normal(94, "unipc/xT", (2, 4, 32, 8)))
    unet, _ = hip_unet(small_cfg(5, 4), "dpm/small.")
    outs = [ldm_pipe(unipc(prediction_type=ptype, solver_order=order), unet)(batch_size=2, num_inference_steps=8, latents=x_T,
                                                                             output_type="torch", fused=fused).cpu()
            for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5


def test_captured_sampler_runs_the_disabled_corrector_rows():
    x_T = T(normal(94, "unipc/xT", (2, 4, 32, 8)))
    unet, _ = hip_unet(small_cfg(5, 4), "dpm/small.")
    kw = dict(batch_size=2, num_inference_steps=8, latents=x_T, output_type="torch")
    off = [ldm_pipe(unipc(disable_corrector=[0, 3]), unet)(fused=fused, **kw).cpu() for fused in (True, False)]
    assert rel_l2(off[0], off[1]) < 1e-5
    assert not torch.equal(off[0], ldm_pipe(unipc(), unet)(**kw).cpu())


def test_captured_upscale_and_pixel_samplers_match_eager_loop(golden):
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    from rangeldm_amd.pipelines import DDPMPipelineRange, LDMUpscalePipelineRange
    g = golden("up")
    unet, _ = hip_unet(small_cfg(12, 4), "dpm/up.")
    vae, _ = hip_vae()
    x_T = T(normal(95, "unipc/up/xT", (2, 4, 32, 8)))
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=unipc(solver_order=3))
    outs = [pipe(image=T(g["up_cond"]).cuda(), condition_encoder=SparseRangeImageEncoder2(), batch_size=2, num_inference_steps=6,
                 latents=x_T, output_type="torch", fused=fused).cpu() for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5
    unet_px, _ = hip_unet(small_cfg(3, 3), "dpm/px.")
    pipe = DDPMPipelineRange(unet=unet_px, scheduler=unipc(solver_order=3))
    x_px = T(normal(96, "unipc/px/xT", (2, 3, 32, 8)))
    outs = [pipe(batch_size=2, num_inference_steps=6, latents=x_px, output_type="torch", fused=fused).cpu() for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5


def test_captured_inpainting_sampler_matches_eager_loop():
    """LDMUpscalePipelineRange with a mask: the in-painting route (masked VAE latents as the condition), the posterior draw injected"""
    from rangeldm_amd.pipelines import LDMUpscalePipelineRange
    unet, _ = hip_unet(small_cfg(9, 4), "unipc/inpaint.")
    vae, _ = hip_vae()
    image = T(normal(97, "unipc/inpaint/image", (2, 2, 128, 32)))
    mask = torch.ones(2, 1, 128, 32)
    mask[:, :, 40:90] = 0
    enc = T(normal(97, "unipc/inpaint/enc", (2, 4, 32, 8))).cuda()
    x_T = T(normal(97, "unipc/inpaint/xT", (2, 4, 32, 8)))
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=unipc())
    outs = [pipe(image=(image * mask).cuda(), mask=mask.cuda(), batch_size=2, num_inference_steps=6, latents=x_T, encode_noise=enc, output_type="torch",
                 fused=fused).cpu() for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5


def test_lanes_and_device_generator(monkeypatch):
    """A sampler split into two lanes, each with its own `last` and history, against one lane; x_T from a rng.DeviceGenerator on the
    captured route and on the eager one (x_T is all the noise this solver takes)."""
    from rangeldm_amd.rng import DeviceGenerator
    x_T = T(normal(98, "unipc/xT4", (4, 4, 32, 8)))
    kw = dict(batch_size=4, num_inference_steps=8, output_type="torch")
    one = ldm_pipe(unipc(solver_order=3))(latents=x_T, **kw).cpu()
    drawn = [ldm_pipe(unipc(solver_order=3))(generator=DeviceGenerator(7), fused=fused, **kw).cpu() for fused in (True, False)]
    assert torch.isfinite(drawn[0]).all() and rel_l2(drawn[0], drawn[1]) < 1e-5 and not torch.equal(drawn[0], one)
    monkeypatch.setenv("RLDM_LANES", "2")
    lanes = ldm_pipe(unipc(solver_order=3))(latents=x_T, **kw).cpu()
    print(f"two lanes vs one: rel-L2 {rel_l2(lanes, one):.3e}")
    assert torch.isfinite(lanes).all() and rel_l2(lanes, one) < TOL_FWD


def test_sampler_keeps_no_state_between_calls():
    x1, x2 = (T(normal(99, f"unipc/xT/{k}", (2, 4, 32, 8))) for k in (1, 2))
    unet, _ = hip_unet(small_cfg(5, 4), "dpm/small.")
    pipe = ldm_pipe(unipc(solver_order=3), unet)
    kw = dict(batch_size=2, num_inference_steps=8, output_type="torch")
    a = pipe(latents=x1, **kw).cpu()
    b = pipe(latents=x2, **kw).cpu()
    c = pipe(latents=x1, **kw).cpu()
    assert len(pipe._fused._cache) == 1 and pipe._fused.captures(next(iter(pipe._fused._cache.values()))[0]) == 1
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert torch.equal(ldm_pipe(unipc(solver_order=3), unet)(latents=x2, **kw).cpu(), b)
    # the rows are part of the sampler's identity: another order at the same step count is another sampler
    pipe.scheduler = unipc(solver_order=2)
    d = pipe(latents=x1, **kw).cpu()
    assert len(pipe._fused._cache) == 2 and not torch.equal(d, a)


# ---- refusals and drivers ---------------------------------------------------------------------------------------------------
def test_guided_and_decoder_guided_sampling_refuse_unipc():
    unet, _ = hip_unet(small_cfg(5, 4), "dpm/small.")
    pipe = ldm_pipe(unipc(), unet)
    known = torch.zeros(2, 2, 128, 32)
    mask = torch.ones(2, 1, 128, 32)
    with pytest.raises(NotImplementedError, match="x0 history"):
        pipe(batch_size=2, num_inference_steps=4, known=known, known_mask=mask, output_type="torch")
    with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
        pipe(batch_size=2, num_inference_steps=4, known=known, known_mask=mask, decoder_guidance=True, output_type="torch")
    # ... and the library itself: a guided program on the UniPC mode
    program = repaint_program(DDIMSchedulerHIP(), 4)
    with pytest.raises(RuntimeError, match="guided sampler runs DDIM"):
        pipe._fused.get(unet, None, pipe.scheduler, 2, 4, _lib.RLDM_SAMPLER_UNIPC, True, 0, program=program)


def test_inference_cli_with_unipc(tmp_path):
    from rangeldm_amd import inference, inference_conditional
    out = tmp_path / "generated"
    inference.main(["--cfg", "RangeLDM", "--samples", "2", "--batch_size", "2", "--scheduler", "unipc", "--steps", "10",
                    "--out", str(out)])
    assert sorted(p.name for p in out.iterdir()) == ["0.bin", "0.png", "0_range.png", "1.bin", "1.png", "1_range.png"]
    assert all(p.stat().st_size > 0 for p in out.iterdir())
    cond = tmp_path / "cond"
    inference_conditional.main(["--cfg", "upsample", "--samples", "2", "--batch_size", "2", "--scheduler", "unipc", "--solver-order", "3",
                                "--steps", "4", "--out", str(cond)])
    assert sorted(p.name for p in (cond / "densification_result").iterdir())[:2] == ["0_seed_0.bin", "0_seed_0.png"]
    with pytest.raises(ValueError, match="solver-order"):
        inference.make_scheduler("ddim", None, solver_order=2)
