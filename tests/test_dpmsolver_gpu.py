"""GPU: DPM-Solver++(2M) -- rldm_sched_dpmsolver_step against numpy, the eager pipeline loop against the oracle networks driven by a
restated scheduler, the captured sampler (RLDM_SAMPLER_DPMSOLVER: the x0 history in conv_out's fused epilogue) against the eager
loop on every route, and the sampling driver."""
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd.config import SchedulerConfig, UNetConfig, VAEConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.schedulers import DPMSolverMultistepSchedulerHIP
from rangeldm_amd.synth import normal, synth_state_dict
from oracle import pipelines as o_pipe, unet as o_unet, vae as o_vae
from tests.hip_util import rel_l2
from tests.test_dpmsolver_host import ref_rows, ref_timesteps
from tests.test_oracle_golden import SGM_SINUSOID, ref_unet_sd

pytestmark = pytest.mark.gpu
TOL_FWD = 1.2e-2     # one network forward, teacher-forced (tests/test_hip_models.py)
TOL_TRAJ = 2e-2      # decoded image at the end of a free-running trajectory
TOL_X0 = 5e-3        # final latent of a full-width free-running sampler
PTYPES = ("epsilon", "v_prediction", "sample")


def T(a):
    return torch.from_numpy(np.asarray(a))


class RestatedDPM:
    """DPM-Solver++(2M) on the host in float64 from the test's own rows (tests/test_dpmsolver_host.py), for the oracle loops."""
    init_noise_sigma = 1.0

    def __init__(self, prediction_type="epsilon", order=2, spacing="leading"):
        self.ptype, self.order, self.spacing = prediction_type, order, spacing

    def set_timesteps(self, n, device=None):
        ts = ref_timesteps(n, self.spacing)
        self.rows, _ = ref_rows(ts, self.order)
        self.timesteps = torch.from_numpy(np.ascontiguousarray(ts))
        self.i, self.x0_prev = 0, None

    def scale_model_input(self, x, t=None):
        return x

    def step(self, out, t, x, generator=None, noise=None):
        a, s, c_x0, c_xt, c_x0p = self.rows[self.i]
        out, x = out.double(), x.double()
        if self.ptype == "epsilon":
            x0 = (x - s * out) / a
        elif self.ptype == "v_prediction":
            x0 = a * x - s * out
        else:
            x0 = out
        prev = c_x0 * x0 + c_xt * x
        if c_x0p != 0:
            prev = prev + c_x0p * self.x0_prev
        self.x0_prev, self.i = x0, self.i + 1
        return SimpleNamespace(prev_sample=prev.float())


def np_x0(ptype, a, s, out, x):
    return {"epsilon": (x - s * out) / a, "v_prediction": a * x - s * out, "sample": out}[ptype]


def hip_unet(cfg, prefix, sd=None):
    from rangeldm_amd.unet import UNet2DModelHIP
    sd = sd if sd is not None else synth_state_dict(unet_param_shapes(cfg), prefix=prefix)
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(sd)
    return m, sd


_VAE = {}


def hip_vae():
    from rangeldm_amd.vae import AutoencoderKLHIP
    if "m" not in _VAE:
        sd = synth_state_dict(vae_param_shapes(VAEConfig()), prefix="vae.")
        m = AutoencoderKLHIP(VAEConfig())
        m.load_state_dict(sd)
        _VAE["m"], _VAE["sd"] = m, sd
    return _VAE["m"], _VAE["sd"]


def small_cfg(in_ch, out_ch):
    return UNetConfig(sample_size=(32, 8), in_channels=in_ch, out_channels=out_ch, block_out_channels=(32, 32, 64, 64))


# ---- the elementwise entry point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", PTYPES)
def test_sched_dpmsolver_step_matches_numpy(ptype):
    sch = DPMSolverMultistepSchedulerHIP(prediction_type=ptype)
    sch.set_timesteps(10)
    rows = sch.coefficients()
    n = 3001                                                  # (not a multiple of the block)
    out, x, x0_prev = (normal(81, f"dpm/{k}", (n,)) for k in ("out", "x", "x0_prev"))
    dev = torch.device("cuda")

    def run(row, hist):
        o, xx = T(out).to(dev), T(x).to(dev)
        prev = torch.empty_like(xx)
        cf = (C.c_float * 5)(*[float(v) for v in row])
        _lib.check(_lib.lib().rldm_sched_dpmsolver_step(sch.prediction_code, cf, C.c_void_p(o.data_ptr()), C.c_void_p(xx.data_ptr()),
                                                        C.c_void_p(hist.data_ptr()), C.c_void_p(prev.data_ptr()), n,
                                                        _lib.stream_ptr(dev)), "rldm_sched_dpmsolver_step")
        torch.cuda.synchronize()
        return prev.cpu().double().numpy(), hist.cpu().double().numpy()

    for i in (0, 4):                                          # a first-order row, a second-order row
        row = rows[i].astype(np.float64)
        assert (row[4] == 0) == (i == 0)
        a, s, c_x0, c_xt, c_x0p = row
        x0 = np_x0(ptype, a, s, out.astype(np.float64), x.astype(np.float64))
        want = c_x0 * x0 + c_xt * x + c_x0p * x0_prev
        hist = T(x0_prev).to(dev) if i else torch.full((n,), float("nan"), device=dev)
        got, hist_after = run(rows[i], hist)
        assert np.isfinite(got).all()                         # (row 0: the NaN history is not read)
        assert np.abs(got - want).max() < 2e-5 * (1 + np.abs(want).max()), i
        assert np.abs(hist_after - x0).max() < 2e-5 * (1 + np.abs(x0).max()), i


# ---- pipelines ---------------------------------------------------------------------------------------------------------------
def test_eager_ldm_loop_matches_oracle():
    """LDMPipelineRange(fused=False) through DPMSolverMultistepSchedulerHIP.step against the oracle UNet and VAE driven by the
    restated scheduler."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = small_cfg(5, 4)
    unet, sd = hip_unet(cfg, "dpm/small.")
    vae, vsd = hip_vae()
    x_T = T(normal(82, "dpm/xT", (2, 4, 32, 8)))
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
    img = pipe(batch_size=2, num_inference_steps=8, latents=x_T, output_type="torch", fused=False).cpu()
    ref = o_pipe.ldm_pipeline(o_vae.OracleVAE(VAEConfig(), vsd), o_unet.OracleUNet(cfg, sd), RestatedDPM(), x_T, 8,
                              pos_encoding=True)
    e = rel_l2(img, ref)
    print(f"eager DPM++ 8 steps vs oracle: rel-L2 {e:.3e}")
    assert torch.isfinite(img).all() and e < 3 * TOL_FWD


@pytest.mark.parametrize("ptype", PTYPES)
def test_captured_ldm_sampler_matches_eager_loop(ptype):
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = small_cfg(5, 4)
    unet, _ = hip_unet(cfg, "dpm/small.")
    vae, _ = hip_vae()
    x_T = T(normal(83, "dpm/xT", (2, 4, 32, 8)))
    outs = []
    for fused in (True, False):
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(SchedulerConfig(prediction_type=ptype)),
                                pos_encoding=True)
        outs.append(pipe(batch_size=2, num_inference_steps=8, latents=x_T, output_type="torch", fused=fused).cpu())
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5


def test_captured_upscale_and_pixel_samplers_match_eager_loop(golden):
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    from rangeldm_amd.pipelines import DDPMPipelineRange, LDMUpscalePipelineRange
    g = golden("up")
    unet, _ = hip_unet(small_cfg(12, 4), "dpm/up.")
    vae, _ = hip_vae()
    x_T = T(normal(84, "dpm/up/xT", (2, 4, 32, 8)))
    pipe = LDMUpscalePipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP())
    outs = [pipe(image=T(g["up_cond"]).cuda(), condition_encoder=SparseRangeImageEncoder2(), batch_size=2, num_inference_steps=6,
                 latents=x_T, output_type="torch", fused=fused).cpu() for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5
    unet_px, _ = hip_unet(small_cfg(3, 3), "dpm/px.")
    pipe = DDPMPipelineRange(unet=unet_px, scheduler=DPMSolverMultistepSchedulerHIP())
    x_px = T(normal(85, "dpm/px/xT", (2, 3, 32, 8)))
    outs = [pipe(batch_size=2, num_inference_steps=6, latents=x_px, output_type="torch", fused=fused).cpu() for fused in (True, False)]
    assert torch.isfinite(outs[0]).all() and rel_l2(outs[0], outs[1]) < 1e-5


def test_separate_launch_tail_and_lanes_match_fused_tail(monkeypatch):
    """rldm_debug_set_flags(Flag.SCHED_LAUNCH) at sampler creation: the scheduler step as sched_step_kernel launches of their own, against
    the step in conv_out's epilogue; and a sampler split into two lanes (each with its own x0 history)."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = small_cfg(5, 4)
    vae, _ = hip_vae()
    x_T = T(normal(86, "dpm/xT4", (4, 4, 32, 8)))
    outs = {}
    for key, flags in (("fused", 0), ("separate", _lib.Flag.SCHED_LAUNCH)):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            unet, _ = hip_unet(cfg, "dpm/small.")
            pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
            outs[key] = pipe(batch_size=4, num_inference_steps=8, latents=x_T, output_type="torch").cpu()
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    assert torch.isfinite(outs["fused"]).all() and rel_l2(outs["separate"], outs["fused"]) < 1e-5
    monkeypatch.setenv("RLDM_LANES", "2")
    unet, _ = hip_unet(cfg, "dpm/small.")
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
    lanes = pipe(batch_size=4, num_inference_steps=8, latents=x_T, output_type="torch").cpu()
    print(f"two lanes vs one: rel-L2 {rel_l2(lanes, outs['fused']):.3e}")
    assert torch.isfinite(lanes).all() and rel_l2(lanes, outs["fused"]) < TOL_FWD


def test_sampler_keeps_no_state_between_calls():
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = small_cfg(5, 4)
    unet, _ = hip_unet(cfg, "dpm/small.")
    vae, _ = hip_vae()
    x1, x2 = (T(normal(87, f"dpm/xT/{k}", (2, 4, 32, 8))) for k in (1, 2))
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
    kw = dict(batch_size=2, num_inference_steps=8, output_type="torch")
    a = pipe(latents=x1, **kw).cpu()
    b = pipe(latents=x2, **kw).cpu()
    c = pipe(latents=x1, **kw).cpu()
    assert len(pipe._fused._cache) == 1
    assert torch.equal(a, c)
    fresh = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
    assert torch.equal(fresh(latents=x2, **kw).cpu(), b)
    # the schedule is part of the sampler's identity: another solver order or spacing at the same step count is another sampler
    pipe.scheduler = DPMSolverMultistepSchedulerHIP(solver_order=1)
    d = pipe(latents=x1, **kw).cpu()
    pipe.scheduler = DPMSolverMultistepSchedulerHIP(timestep_spacing="trailing")
    e = pipe(latents=x1, **kw).cpu()
    assert len(pipe._fused._cache) == 3
    assert not torch.equal(d, a) and not torch.equal(e, a)


# ---- full width ------------------------------------------------------------------------------------------------------------
def test_batch16_sampler_clusters_match_launch_per_layer():
    """BASELINE config 2 at its real batch, 20 DPM++ steps through the captured sampler: the persistent clusters against
    rldm_debug_set_flags(Flag.NO_CLUSTERS) (one launch per layer).  Same kernels on the same operands: identical images."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    x_T = T(normal(88, "dpm/b16/xT", (16, 4, 256, 16)))
    outs = []
    for flags in (0, _lib.Flag.NO_CLUSTERS):
        _lib.lib().rldm_debug_set_flags(flags)
        try:
            unet, _ = hip_unet(UNetConfig(), "")
            vae, _ = hip_vae()
            pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
            outs.append(pipe(batch_size=16, num_inference_steps=20, latents=x_T, output_type="torch").cpu())
        finally:
            _lib.lib().rldm_debug_set_flags(0)
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


def test_full_width_sampler_matches_oracle_loop():
    """The headline model at batch 2, 10 DPM++ steps, free-running: the captured sampler against the oracle's fp32 loop with the
    restated scheduler (the weights and gates of tests/test_hip_models.py's 50-step full-width test)."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = UNetConfig(**SGM_SINUSOID)
    sd = ref_unet_sd(cfg, "ref/full.")
    unet, _ = hip_unet(cfg, "", sd=sd)
    vae, vsd = hip_vae()
    x_T = T(normal(89, "dpm/full/xT", (2, 4, 256, 16)))
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DPMSolverMultistepSchedulerHIP(), pos_encoding=True)
    h = pipe._fused.get(unet, vae, pipe.scheduler, 2, 10, _lib.RLDM_SAMPLER_DPMSOLVER, True, 0)
    img = torch.empty((2, 2, 1024, 64), device="cuda")
    lat = torch.empty((2, 4, 256, 16), device="cuda")
    pipe._fused.run(h, x_T.cuda().contiguous(), None, None, img, latents_out=lat)
    ovae = o_vae.OracleVAE(VAEConfig(), vsd)
    ref_lat = o_pipe.ldm_pipeline(None, o_unet.OracleUNet(cfg, sd), RestatedDPM(), x_T, 10, pos_encoding=True, decode=False)
    ref_img = ovae.decode(ref_lat / VAEConfig().scaling_factor).sample
    e_lat, e_img = rel_l2(lat.cpu(), ref_lat), rel_l2(img.cpu(), ref_img)
    print(f"10-step DPM++ full width: final latent rel-L2 {e_lat:.3e}, decoded image rel-L2 {e_img:.3e}")
    assert e_lat < TOL_X0 and e_img < TOL_TRAJ
    assert torch.equal(pipe(batch_size=2, num_inference_steps=10, latents=x_T, output_type="torch"), img)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
def test_inference_cli_with_dpmsolver(tmp_path):
    from rangeldm_amd import inference, inference_conditional
    out = tmp_path / "generated"
    inference.main(["--cfg", "RangeLDM", "--samples", "2", "--batch_size", "2", "--scheduler", "dpmsolver++", "--steps", "4",
                    "--out", str(out)])
    assert sorted(p.name for p in out.iterdir()) == ["0.bin", "0.png", "0_range.png", "1.bin", "1.png", "1_range.png"]
    assert all(p.stat().st_size > 0 for p in out.iterdir())
    cond = tmp_path / "cond"
    inference_conditional.main(["--cfg", "upsample", "--samples", "2", "--batch_size", "2", "--scheduler", "dpmsolver++",
                                "--steps", "4", "--out", str(cond)])
    assert sorted(p.name for p in (cond / "densification_result").iterdir())[:2] == ["0_seed_0.bin", "0_seed_0.png"]
