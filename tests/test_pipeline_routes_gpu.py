"""GPU: which route a pipeline call takes -- the entry point of the fused sampler, which of its arguments are null, or the eager loop --
how many draws of a rng.DeviceGenerator it consumes, and how many samplers the sequence of calls created.  Nothing but Python-level
calls is looked at: `pipe._fused` is replaced by a recorder that delegates to the real _FusedSampler."""
import numpy as np
import pytest
import torch

from rangeldm_amd import rng
from rangeldm_amd.encoders import SparseRangeImageEncoder2
from rangeldm_amd.pipelines import DDIMPipelineRange, DDPMPipelineRange, LDMPipelineRange, LDMUpscalePipelineRange
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP, repaint_program
from rangeldm_amd.synth import normal
from tests.hip_util import hip_unet, hip_vae, small_cfg

pytestmark = pytest.mark.gpu
B, STEPS, OFFSET = 2, 4, 6
LAT = (B, 4, 32, 8)
# the tensor arguments of each entry point after the handle, by name (ints -- seed, draw, sample_offset -- are not listed)
ARGS = {"run": ("x_T", "step_noise", "cond", "out"),
        "run_guided": ("x_T", "step_noise", "known", "mask", "known_noise", "renoise_noise", "out"),
        "run_rng": ("x_T", None, None, None, "cond", "out"),
        "run_guided_rng": ("x_T", None, None, None, "known", "mask", "out")}


class Recorder:
    """Stands in for pipe._fused: every run* call is noted as (name, the set of its tensor arguments that were None), then made."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if name not in ARGS:
            return attr

        def call(h, *args, **kw):
            null = {n for n, a in zip(ARGS[name], args) if n is not None and a is None}
            self.calls.append((name, frozenset(null)))
            return attr(h, *args, **kw)
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def N(seed, tag, shape):
    return torch.from_numpy(normal(seed, tag, shape)).cuda()


def recorded(pipe):
    pipe._fused = Recorder(pipe._fused)
    return pipe


def route(pipe, gen=None, **kw):
    """One call -> its recorded fused calls ([] = the eager loop); with a DeviceGenerator, sample_offset is passed along."""
    if isinstance(gen, rng.DeviceGenerator):
        kw["sample_offset"] = OFFSET
    out = pipe(generator=gen, batch_size=B, num_inference_steps=STEPS, output_type="torch", **kw)
    first = out[0] if isinstance(out, (tuple, list)) else out
    assert torch.isfinite(first).all()
    return pipe._fused.take()


def one(name, *null):
    return [(name, frozenset(null))]


def test_ddpm_pipeline_routes():
    unet = hip_unet(small_cfg(3, 3), "routes/px.")
    shape = (B, 3, 32, 8)
    x_T, zs = N(1, "routes/px/xT", shape), N(2, "routes/px/zs", (STEPS, *shape))
    pipe = recorded(DDPMPipelineRange(unet=unet, scheduler=DDPMSchedulerHIP()))
    gen = rng.DeviceGenerator(3)
    # the graph draws x_T and the rows: the only route with a null x_T
    assert route(pipe, gen) == one("run_rng", "x_T", "cond") and gen.draw == 1
    assert route(pipe, gen, latents=x_T) == one("run_rng", "cond") and gen.draw == 2
    assert route(pipe, gen, step_noise=zs) == one("run", "cond") and gen.draw == 3
    assert route(pipe, torch.Generator().manual_seed(1)) == one("run", "cond")
    assert route(pipe, None, latents=x_T, step_noise=zs) == one("run", "cond")
    assert len(pipe._fused._cache) == 1
    assert route(pipe, gen, fused=False) == [] and gen.draw == 4
    assert route(pipe, None, latents=x_T, step_noise=zs, fused=False) == []
    assert len(pipe._fused._cache) == 1
    # DPM-Solver++: the explicit entry point without a noise tensor, whatever the generator
    pipe = recorded(DDPMPipelineRange(unet=unet, scheduler=DPMSolverMultistepSchedulerHIP()))
    gen = rng.DeviceGenerator(3)
    assert route(pipe, gen) == one("run", "step_noise", "cond") and gen.draw == 1
    assert route(pipe, torch.Generator().manual_seed(1)) == one("run", "step_noise", "cond")
    assert len(pipe._fused._cache) == 1
    # any other scheduler: eager
    pipe = recorded(DDPMPipelineRange(unet=unet, scheduler=DDIMSchedulerHIP()))
    assert route(pipe, gen) == [] and gen.draw == 2 and len(pipe._fused._cache) == 0


def test_ddim_pipeline_routes():
    pipe = recorded(DDIMPipelineRange(unet=hip_unet(small_cfg(5, 4), "routes/small."), scheduler=DDPMSchedulerHIP(), pos_encoding=True))
    gen = rng.DeviceGenerator(4)
    assert route(pipe, gen) == one("run", "step_noise", "cond") and gen.draw == 1
    assert route(pipe, torch.Generator().manual_seed(1)) == one("run", "step_noise", "cond")
    assert route(pipe, torch.Generator().manual_seed(1), eta=0.5) == []
    assert route(pipe, gen, fused=False) == [] and gen.draw == 2
    with pytest.raises(NotImplementedError, match="torch generator"):
        route(pipe, gen, eta=0.5)
    assert gen.draw == 3                                     # the draw is consumed before the refusal
    assert len(pipe._fused._cache) == 1
    # guided (DDIM rows: no step noise)
    known = N(5, "routes/ddim/known", LAT)
    mask = torch.ones((B, 1, 32, 8), device="cuda")
    mask[:, :, 8:20] = 0
    rows = len(repaint_program(pipe.scheduler, STEPS, 2, 2)[0])
    nk = N(6, "routes/ddim/nk", (rows, *LAT))
    g = dict(known=known, known_mask=mask, jump_length=2, jump_n_sample=2)
    assert route(pipe, gen, **g) == one("run_guided_rng", "out") and gen.draw == 4
    assert route(pipe, gen, known_noise=nk, **g) == one("run_guided", "step_noise", "out") and gen.draw == 5
    assert route(pipe, torch.Generator().manual_seed(1), **g) == one("run_guided", "step_noise", "out")
    assert route(pipe, gen, fused=False, **g) == [] and gen.draw == 6
    assert len(pipe._fused._cache) == 2
    # jump_n_sample = 1: no row re-noises, so no re-noise tensor is built
    assert route(pipe, torch.Generator().manual_seed(1), known=known, known_mask=mask) == one("run_guided", "step_noise", "renoise_noise", "out")
    assert len(pipe._fused._cache) == 3


def test_ldm_pipeline_routes():
    vae, unet = hip_vae(), hip_unet(small_cfg(5, 4), "routes/small.")
    x_T, zs = N(7, "routes/ldm/xT", LAT), N(8, "routes/ldm/zs", (STEPS, *LAT))
    pipe = recorded(LDMPipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True))
    gen = rng.DeviceGenerator(5)
    assert route(pipe, gen) == one("run_rng", "cond") and gen.draw == 1              # WITH x_T, drawn beforehand
    assert route(pipe, gen, step_noise=zs) == one("run", "cond") and gen.draw == 2
    assert route(pipe, torch.Generator().manual_seed(1)) == one("run", "cond")
    assert route(pipe, None, latents=x_T, step_noise=zs) == one("run", "cond")
    assert route(pipe, gen, fused=False) == [] and gen.draw == 3
    images = pipe(generator=gen, sample_offset=OFFSET, batch_size=B, num_inference_steps=STEPS, final_only=False)
    assert pipe._fused.take() == [] and gen.draw == 4 and len(images) == STEPS + 1
    assert len(pipe._fused._cache) == 1
    # guided, DDPM rows
    known = N(9, "routes/ldm/known", (B, 2, 128, 32)) * 0.5
    mask = torch.ones((B, 1, 128, 32), device="cuda")
    mask[:, :, 20:52] = 0
    g = dict(known=known, known_mask=mask, jump_length=2, jump_n_sample=2)
    rows = len(repaint_program(pipe.scheduler, STEPS, 2, 2)[0])
    nr = N(10, "routes/ldm/nr", (rows, *LAT))
    assert route(pipe, gen, **g) == one("run_guided_rng") and gen.draw == 5
    assert route(pipe, gen, renoise_noise=nr, **g) == one("run_guided") and gen.draw == 6
    assert route(pipe, torch.Generator().manual_seed(1), **g) == one("run_guided")
    assert route(pipe, gen, fused=False, **g) == [] and gen.draw == 7
    assert len(pipe._fused._cache) == 2
    # a one-row DDPM program (sigma == 0 on its only row) still gets a step-noise tensor; nothing else is built
    out = pipe(generator=torch.Generator().manual_seed(1), batch_size=B, num_inference_steps=1, output_type="torch", known=known, known_mask=mask)
    assert torch.isfinite(out).all() and pipe._fused.take() == one("run_guided", "known_noise", "renoise_noise")
    assert len(pipe._fused._cache) == 3
    # DDIM and DPM-Solver++: the explicit entry point, no noise tensor; DDIM with eta != 0 is eager
    for sch in (DDIMSchedulerHIP(), DPMSolverMultistepSchedulerHIP()):
        pipe = recorded(LDMPipelineRange(vae=vae, unet=unet, scheduler=sch, pos_encoding=True))
        gen = rng.DeviceGenerator(5)
        assert route(pipe, gen) == one("run", "step_noise", "cond") and gen.draw == 1
        assert route(pipe, torch.Generator().manual_seed(1), eta=0.5) == ([] if isinstance(sch, DDIMSchedulerHIP) else one("run", "step_noise", "cond"))
        assert len(pipe._fused._cache) == 1
    # decoder guidance: the eager loop of guidance.py, one draw
    pipe = recorded(LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True))
    gen = rng.DeviceGenerator(5)
    dmask = torch.zeros((B, 1, 128, 32), device="cuda")
    dmask[..., 2::4] = 1
    assert route(pipe, gen, decoder_guidance=True, known=known, known_mask=dmask) == [] and gen.draw == 1
    assert len(pipe._fused._cache) == 0
    # ... and its refusals come before a model is touched or anything is drawn
    bare = LDMPipelineRange(vae=None, unet=None, scheduler=DDPMSchedulerHIP())
    with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
        bare(generator=gen, decoder_guidance=True, known=known, known_mask=dmask)
    assert gen.draw == 1


def test_upscale_pipeline_routes():
    vae = hip_vae()
    cond = N(11, "routes/up/cond", (B, 2, 128, 8))
    zs = N(12, "routes/up/zs", (STEPS, *LAT))
    up = dict(image=cond, condition_encoder=SparseRangeImageEncoder2())
    pipe = recorded(LDMUpscalePipelineRange(vae=vae, unet=hip_unet(small_cfg(12, 4), "routes/up."), scheduler=DDPMSchedulerHIP()))
    gen = rng.DeviceGenerator(6)
    assert route(pipe, gen, **up) == one("run_rng") and gen.draw == 1
    assert route(pipe, gen, step_noise=zs, **up) == one("run") and gen.draw == 2
    assert route(pipe, torch.Generator().manual_seed(1), **up) == one("run")
    assert route(pipe, gen, fused=False, **up) == [] and gen.draw == 3
    assert len(pipe._fused._cache) == 1
    for sch in (DDIMSchedulerHIP(), DPMSolverMultistepSchedulerHIP()):
        pipe = recorded(LDMUpscalePipelineRange(vae=vae, unet=pipe.unet, scheduler=sch))
        gen = rng.DeviceGenerator(6)
        assert route(pipe, gen, **up) == one("run", "step_noise") and gen.draw == 1
        assert route(pipe, torch.Generator().manual_seed(1), eta=0.5, **up) == ([] if isinstance(sch, DDIMSchedulerHIP) else one("run", "step_noise"))
        assert len(pipe._fused._cache) == 1
    # in-painting: a DeviceGenerator gives the posterior a draw of its own, before the sampler's, unless encode_noise is given
    image = N(13, "routes/inp/image", (B, 2, 128, 32)) * 0.5
    mask = -torch.ones((B, 1, 128, 32), device="cuda")
    mask[:, :, 30:60] = 1
    pipe = recorded(LDMUpscalePipelineRange(vae=vae, unet=hip_unet(small_cfg(9, 4), "routes/inp."), scheduler=DDPMSchedulerHIP()))
    gen = rng.DeviceGenerator(6)
    a = pipe(image=image, mask=mask, generator=gen, sample_offset=OFFSET, batch_size=B, num_inference_steps=STEPS)
    assert pipe._fused.take() == one("run_rng") and gen.draw == 2
    enc = rng.randn(LAT, gen.at(0), OFFSET)                  # the posterior's draw is draw 0, the sampler's draw 1
    twin = rng.DeviceGenerator(6).set_state((6, 1))
    b = pipe(image=image, mask=mask, generator=twin, sample_offset=OFFSET, encode_noise=enc, batch_size=B, num_inference_steps=STEPS)
    assert pipe._fused.take() == one("run_rng") and twin.draw == 2
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert route(pipe, gen, image=image, mask=mask, fused=False) == [] and gen.draw == 4
    assert len(pipe._fused._cache) == 1
