"""Sampling pipelines with the reference's names and `__call__` signatures (ldm/pipelines.py):
DDPMPipelineRange :34-117, DDIMPipelineRange :144-258, LDMPipelineRange :282-383, LDMUpscalePipelineRange :414-519.

Two execution modes, same results:
  * `fused=True` (default): the whole loop -- conv_in input packing (pos-encoding / condition concat), UNet, scheduler
    step, VAE decode -- runs as HIP graphs inside librangeldm_hip (`rldm_sample`); one host call per batch.
  * `fused=False`: the reference's Python loop verbatim, each `unet(...)` / `scheduler.step(...)` / `vae.decode(...)`
    going through the C ABI individually (this is what "ldm/pipelines.py calls it unchanged" exercises).

`generator=rng.DeviceGenerator(seed)` (with `sample_offset=`): the noise comes from the counter-based generator of csrc/rng.hip.  A
pipeline call consumes ONE draw d: x_T is (d, purpose 0, row 0), the step noise of row r (d, 1, r), the known-region noise (d, 2, r),
the re-noise (d, 3, r); sample b of the call is sample_offset + b.  fused=True draws the rows inside the step graph (rldm_sample_rng /
rldm_sample_guided_rng: one row buffer per lane, no [rows, B, ...] tensor); fused=False draws the same values row by row with
rng.randn.  Explicit latents= / step_noise= / known_noise= / renoise_noise= keep priority.  DDIM and DPM-Solver++ draw only x_T.
"""
import ctypes as C
import inspect

import numpy as np
import torch

from . import _lib
from .rng import DeviceGenerator, randn, randn_rows
from .schedulers import (DDIMSchedulerHIP, DDPMSchedulerHIP, MultistepSchedulerBase, guided_step, randn_tensor, repaint_program,
                         sampler_mode)


class ImagePipelineOutput:
    def __init__(self, images):
        self.images = images


def _pos_channel(B, W, H, device, dtype=torch.float32):
    """The position channel (B, 1, W, H) concatenated to the UNet's input: 1 on the first row, 0 elsewhere (ldm/pipelines.py:229-231)."""
    pos_encoding = torch.zeros([B, 1, W, H], device=device, dtype=dtype)
    pos_encoding[:, :, 0, :] = 1
    return pos_encoding


class _CallNoise:
    """The noise of ONE pipeline call, made from (generator, sample_offset, device) at the top of the call; the only code that knows
    which kind of generator it holds.

    None / a torch generator / a list of them: x_T is one randn_tensor, the [rows, ...] tensor of a purpose one randn_tensor per row
    that needs one, in row order (a guided call: step, known, re-noise), and an eager loop lets the scheduler draw.
    A rng.DeviceGenerator: the call consumes ONE draw d here; x_T is (d, purpose 0, row 0), row r of purpose P is (d, P, r), sample b of
    the call is sample_offset + b -- the same values whether a tensor is built (randn_rows), an eager loop asks row by row, or the
    captured loop draws them itself (`in_graph`).  A tensor the caller gives always wins, purpose by purpose."""

    def __init__(self, generator, sample_offset, device):
        self.generator, self.sample_offset, self.device = generator, sample_offset, device
        self._counter = isinstance(generator, DeviceGenerator)
        self.draw = generator.next_draw() if self._counter else None

    @staticmethod
    def own_draw(shape, generator, sample_offset, device):
        """Noise that gets a whole draw of a DeviceGenerator to itself, consumed now (the in-painting posterior, before the sampler's
        draw); None for a torch generator, which its consumer draws from in its own turn."""
        return randn(shape, generator, sample_offset, device) if isinstance(generator, DeviceGenerator) else None

    @property
    def torch_generator(self):
        """What a scheduler or latent_dist.sample may draw from by itself: the torch generator(s), None for a DeviceGenerator."""
        return None if self._counter else self.generator

    def refuse_variance_noise(self, eta):
        if self._counter and eta != 0.0:
            raise NotImplementedError("DDIM with eta > 0 draws its variance noise from a torch generator")

    def x_T(self, shape, given, on_host):
        """`given`, else the call's x_T.  A torch draw is made on the CPU when `on_host` (the latent pipelines, as ldm/pipelines.py:329-333)
        and on the device otherwise (the pixel pipelines, which also check the shape of a given one)."""
        if given is not None:
            if not on_host and tuple(given.shape) != tuple(shape):
                raise ValueError(f"latents shape {tuple(given.shape)} != {shape}")
            return given
        if self._counter:
            return randn(shape, self.generator.at(self.draw), self.sample_offset, self.device)
        if on_host:
            return randn_tensor(shape, generator=self.generator)
        return randn_tensor(shape, generator=self.generator, device=self.device, dtype=torch.float32)

    def rows(self, purpose, need, shape, given=None, name=None, always=False):
        """The [len(need), *shape] fp32 device tensor of `purpose`: `given` (with `name`: shape-checked), else drawn for the rows r with
        need[r] -- a torch generator leaves the others 0.  None when no row needs one, a zero tensor with `always`."""
        n = len(need)
        if given is not None:
            if name is not None and tuple(given.shape) != (n, *shape):
                raise ValueError(f"{name} shape {tuple(given.shape)} != {(n, *shape)} (one slice per row of the program)")
            return given.to(self.device, torch.float32).contiguous()
        if not any(need):
            return torch.zeros((n, *shape), device=self.device, dtype=torch.float32) if always else None
        if self._counter:
            return randn_rows(n, shape, self.generator, self.draw, purpose, self.sample_offset, self.device)
        zs = torch.zeros((n, *shape), device=self.device, dtype=torch.float32)
        for r in np.nonzero(need)[0]:
            zs[r] = randn_tensor(shape, generator=self.generator, device=self.device, dtype=torch.float32)
        return zs

    def row(self, purpose, r, shape, given=None):
        """Row r of `purpose` for an eager loop: given[r], else the DeviceGenerator's row; None = let the scheduler draw."""
        if given is not None:
            return given[r]
        if self._counter:
            return randn(shape, self.generator.at(self.draw, purpose, r), self.sample_offset, self.device)
        return None

    def in_graph(self, fused, *given):
        """May the captured loop draw the rows itself?  A DeviceGenerator, the fused route, and none of the purposes it needs given;
        `seed_draw_offset` is then what the entry point takes in place of the tensors."""
        return self._counter and fused and all(g is None for g in given)

    @property
    def seed_draw_offset(self):
        return (self.generator.seed, self.draw, self.sample_offset)


def latent_known_mask(known_mask, downscale):
    """Pixel mask (B, 1, W, H), 1 / True = known -> latent mask (B, 1, W / f, H / f) fp32: a latent pixel is known only if its
    whole f x f footprint is (a min-pool).  A mask that leaves some sample without one fully known latent pixel -- every 4th beam
    does -- cannot guide a latent sampler: ValueError."""
    m = (known_mask.to(torch.float32) > 0.5).to(torch.float32)
    if m.dim() != 4 or m.shape[1] != 1 or m.shape[2] % downscale or m.shape[3] % downscale:
        raise ValueError(f"known_mask must be (B, 1, W, H) with W, H multiples of {downscale}; got {tuple(m.shape)}")
    lat = -torch.nn.functional.max_pool2d(-m, kernel_size=downscale)
    if bool((lat.flatten(1).sum(1) == 0).any()):
        raise ValueError(f"known_mask leaves no latent pixel whose whole {downscale} x {downscale} footprint is known (a beam-subsampling "
                         "mask does that): guide the pixel-space pipeline (DDIMPipelineRange, RangeDM) instead")
    return lat


class _FusedSampler:
    """Owns one rldm_sampler per (batch, steps, mode, pos_encoding, cond_channels, eta, schedule, guided, plan_flags)."""

    def __init__(self):
        self._cache = {}

    def get(self, unet, vae, scheduler, batch, steps, mode, pos_encoding, cond_channels, eta=0.0, program=None, plan_flags=0):
        # keyed by the model objects themselves (kept alive by the cache entry, so an id is never reused for another
        # model); weights reloaded through load_state_dict are picked up by the library: rldm_sample re-plans and
        # re-captures when the model's generation counter moved (include/rangeldm_hip.h, rldm_unet_finalize)
        # ... and by the schedule itself (timesteps and coefficient rows): two schedulers of one kind and step count can differ
        # in their spacing or solver order
        # `program` = (timesteps, [rows][9] table) of schedulers.repaint_program: a guided sampler, whose num_steps is its row count
        # plan_flags: rldm_sampler_config::plan_flags (_lib.Flag bits scoped to this sampler)
        pred = int(getattr(scheduler, "prediction_code", 0))
        guided = program is not None
        if guided:
            ts = np.ascontiguousarray(program[0].numpy().astype(np.int64))
            coef = np.ascontiguousarray(program[1], dtype=np.float32)
            steps = len(ts)
        else:
            scheduler.set_timesteps(steps)
            ts = np.ascontiguousarray(scheduler.timesteps.numpy().astype(np.int64))
            coef = scheduler.sampler_table(eta if mode == _lib.RLDM_SAMPLER_DDIM else 0.0)
        key = (id(unet), id(vae), batch, steps, mode, bool(pos_encoding), cond_channels, float(eta), pred, ts.tobytes(),
               coef.tobytes(), guided, int(plan_flags))
        ent = self._cache.get(key)
        if ent is not None:
            return ent[0]
        cfg = _lib.SamplerConfigC()
        cfg.batch, cfg.num_steps, cfg.mode = batch, steps, mode
        cfg.pos_encoding = 1 if pos_encoding else 0
        cfg.cond_channels = cond_channels
        cfg.prediction_type = pred
        cfg.guided = 1 if guided else 0
        cfg.plan_flags = int(plan_flags)
        cfg.coef = coef.ctypes.data_as(C.POINTER(C.c_float))
        cfg.timesteps = ts.ctypes.data_as(C.POINTER(C.c_int64))
        h = C.c_void_p()
        _lib.check(_lib.lib().rldm_sampler_create(unet._h, vae._h if vae is not None else None, C.byref(cfg),
                                                  C.byref(h)), "rldm_sampler_create")
        self._cache[key] = (h, unet, vae)
        return h

    def _call(self, entry, h, x_T, args, out, latents_out, check):
        """The one call into the library, `entry`(h, x_T, *args, out, latents_out, stream): every tensor (or None) goes as its pointer,
        every other argument as an int, on the current stream of the tensors' device.
        `check` (default): wait for it and raise RuntimeError if the self-check of its persistent launches tripped -- the reference's
        contract is a correct tensor or an exception (ldm/pipelines.py:218-222,463-464); the failed call's outputs are NaN-marked on the
        device either way, and the sampler has then already rebuilt itself as one launch per layer, so calling again works.
        check=False keeps the call asynchronous (throughput loops that ask `status(h)` themselves before they use the images)."""
        args = (x_T, *args, out, latents_out)
        dev = next(a.device for a in args if torch.is_tensor(a))
        _lib.check(getattr(_lib.lib(), entry)(h, *(_lib.ptr(a) if a is None or torch.is_tensor(a) else int(a) for a in args),
                                              _lib.stream_ptr(dev)), entry)
        if check:
            self.status(h)

    def run(self, h, x_T, step_noise, cond, out, latents_out=None, check=True):
        """One rldm_sample call; `check` as in _call."""
        self._call("rldm_sample", h, x_T, (step_noise, cond), out, latents_out, check)

    def run_guided(self, h, x_T, step_noise, known, mask, known_noise, renoise_noise, out, latents_out=None, check=True):
        """One rldm_sample_guided call on a sampler made with `program`."""
        self._call("rldm_sample_guided", h, x_T, (step_noise, known, mask, known_noise, renoise_noise), out, latents_out, check)

    def run_rng(self, h, x_T, seed, draw, sample_offset, cond, out, latents_out=None, check=True):
        """One rldm_sample_rng call: (seed, draw, sample_offset) in place of step_noise; x_T None = drawn (purpose 0)."""
        self._call("rldm_sample_rng", h, x_T, (seed, draw, sample_offset, cond), out, latents_out, check)

    def run_guided_rng(self, h, x_T, seed, draw, sample_offset, known, mask, out, latents_out=None, check=True):
        """One rldm_sample_guided_rng call on a sampler made with `program`."""
        self._call("rldm_sample_guided_rng", h, x_T, (seed, draw, sample_offset, known, mask), out, latents_out, check)

    def captures(self, h):
        """rldm_debug_sampler_captures: step graphs this sampler has captured so far."""
        return int(_lib.lib().rldm_debug_sampler_captures(h))

    def status(self, h):
        """rldm_sampler_status: waits for the sampler's last call; raises if its outputs are invalid."""
        _lib.check(_lib.lib().rldm_sampler_status(h), "rldm_sample (self-check of the persistent launches)")

    def status_all(self):
        for ent in self._cache.values():
            self.status(ent[0])

    def __del__(self):
        try:
            for ent in self._cache.values():
                _lib.lib().rldm_sampler_destroy(ent[0])
        except Exception:
            pass


class _PipelineBase:
    def __init__(self):
        self._fused = _FusedSampler()
        self._progress = {}

    def register_modules(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def device(self):
        return self.unet.device

    @property
    def _execution_device(self):
        return self.unet.device

    def to(self, device=None, *a, **k):
        return self

    def save_pretrained(self, output_dir):
        """`pipeline.save_pretrained(args.output_dir)` (ldm/train_unconditional.py:675): unet/, vae/, scheduler/ and
        model_index.json in the layout ldm/inference.py:46-52 reads back."""
        import os
        self.unet.save_pretrained(os.path.join(output_dir, "unet"))
        vae = getattr(self, "vae", None)
        if vae is not None:
            vae.save_pretrained(os.path.join(output_dir, "vae"))
        self.scheduler.save_pretrained(os.path.join(output_dir, "scheduler"))
        import json
        sched = self.scheduler._DIFFUSERS_NAME if isinstance(self.scheduler, MultistepSchedulerBase) else "DDPMScheduler"
        index = {"_class_name": type(self).__name__, "_diffusers_version": "0.21.0",
                 "unet": ["diffusers", "UNet2DModel"], "scheduler": ["diffusers", sched]}
        if vae is not None:
            index["vae"] = ["diffusers", "AutoencoderKL"]
        with open(os.path.join(output_dir, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2, sort_keys=True)

    def set_progress_bar_config(self, **kw):
        self._progress = kw

    def progress_bar(self, iterable):
        return iterable

    @staticmethod
    def _finish(image, output_type, return_dict):
        if output_type == "torch":
            return image
        image = (image / 2 + 0.5).clamp(0, 1)
        image = image.cpu().permute(0, 2, 3, 1).numpy()
        if output_type == "pil":
            raise NotImplementedError("output_type='pil' (PIL is not part of the hot path); use 'torch' or 'np'")
        if not return_dict:
            return (image,)
        return ImagePipelineOutput(images=image)

    def _draw_step_noise(self, n_steps, timesteps, shape, generator, device):
        """The [n_steps, *shape] step noise `generator` gives: one randn per step with t > 0, in loop order."""
        return _CallNoise(generator, 0, device).rows(1, [int(t) > 0 for t in timesteps], shape, always=True)

    def _sample_fused(self, shape, x_T, noise, step_noise, steps, check, vae=None, cond=None, pos_encoding=False):
        """The fused unguided route of all four pipelines: x_T (None: the captured loop draws it) -> the decoded images with a VAE, the
        final sample without.  An ancestral (DDPM) sampler takes its step noise from the captured loop itself when `noise` allows, else
        as a [steps, *shape] tensor: `step_noise`, or one draw per step with t > 0 in loop order.  The reference's latent pipelines call
        `scheduler.step` without a generator (ldm/pipelines.py:362,502), i.e. they draw from the unseeded global RNG of the device;
        here the caller's generator seeds the step noise as well (after x_T), so a seeded call is reproducible."""
        sch = self.scheduler
        mode = sampler_mode(sch)
        ancestral = mode == _lib.RLDM_SAMPLER_DDPM
        in_graph = ancestral and noise.in_graph(True, step_noise)
        zs = None
        if ancestral and not in_graph:
            zs = noise.rows(1, [int(t) > 0 for t in sch.timesteps], shape, step_noise, always=True)
        h = self._fused.get(self.unet, vae, sch, shape[0], steps, mode, pos_encoding, 0 if cond is None else cond.shape[1])
        out_shape = shape
        if vae is not None:
            f = vae._cfg.downscale
            out_shape = (shape[0], vae._cfg.out_channels, shape[2] * f, shape[3] * f)
        out = torch.empty(out_shape, device=self.device, dtype=torch.float32)
        x_T = None if x_T is None else x_T.float().contiguous()
        cond = None if cond is None else cond.float().contiguous()
        if in_graph:
            self._fused.run_rng(h, x_T, *noise.seed_draw_offset, cond, out, check=check)
        else:
            self._fused.run(h, x_T, zs, cond, out, check=check)
        return out

    def _latent_loop(self, latents, extra, noise, step_noise, eta, images=None):
        """The eager loop of the latent pipelines (ldm/pipelines.py:340-383, 487-519): scale, concatenate the `extra` input channels (None:
        none), UNet, scheduler step -- an ancestral one with `noise`'s row -- and the final decode, which is returned.  `images`: a
        list that receives the decode of every step's input latents (final_only=False)."""
        sch, sf = self.scheduler, self.vae.config.scaling_factor
        shape = tuple(latents.shape)
        extra_kwargs = {"eta": eta} if "eta" in set(inspect.signature(sch.step).parameters.keys()) else {}
        ancestral = isinstance(sch, DDPMSchedulerHIP)
        for i, t in enumerate(self.progress_bar(sch.timesteps)):
            if images is not None:
                images.append(self.vae.decode(latents / sf).sample)
            latent_model_input = sch.scale_model_input(latents, t)
            if extra is not None:
                latent_model_input = torch.cat([latent_model_input, extra], dim=1)
            noise_prediction = self.unet(latent_model_input, t).sample
            kw = dict(extra_kwargs)
            z = noise.row(1, i, shape, step_noise) if ancestral else None
            if z is not None:
                kw["noise"] = z
            latents = sch.step(noise_prediction, t, latents, **kw).prev_sample
        return self.vae.decode(latents / sf).sample

    def _guided_latents(self, vae, x_T, z0, mask, num_inference_steps, jump_length, jump_n_sample, noise, step_noise, known_noise,
                        renoise_noise, fused, check, out=None):
        """The guided loop (schedulers.repaint_program) on the unconditional UNet: x_T, z0 (B, C, W, H) and mask (B, 1, W, H) at the
        UNet's sample resolution -> the final sample; with `out` (and a VAE, fused) the decoded images are written as well.
        Noise not injected comes from `noise` (_CallNoise) in this order: the step noise (rows with sigma != 0), the known-region noise
        (rows with kb != 0), the re-noise (rows that jump); tensors are built only for purposes some row needs, and with nothing
        injected the fused loop may draw the rows itself."""
        dev = self.device
        sch = self.scheduler
        ts, table = repaint_program(sch, num_inference_steps, jump_length, jump_n_sample)
        rows, shape = len(ts), tuple(x_T.shape)
        mode = sampler_mode(sch)
        in_graph = noise.in_graph(fused, step_noise, known_noise, renoise_noise)
        zs = nk = nr = None
        if not in_graph:
            # (a one-row DDPM program: sigma == 0, the fused sampler still asks for the tensor)
            zs = noise.rows(1, table[:, 4] != 0.0, shape, step_noise, "step_noise", always=fused and mode == _lib.RLDM_SAMPLER_DDPM)
            nk = noise.rows(2, table[:, 6] != 0.0, shape, known_noise, "known_noise")
            nr = noise.rows(3, (table[:, 7] != 1.0) | (table[:, 8] != 0.0), shape, renoise_noise, "renoise_noise")
        x = x_T.to(dev, torch.float32).contiguous()
        z0 = z0.to(dev, torch.float32).contiguous()
        mask = mask.to(dev, torch.float32).expand(shape[0], 1, *shape[2:]).contiguous()
        if z0.shape != x.shape:
            raise ValueError(f"known sample {tuple(z0.shape)} != sample shape {shape}")
        if fused:
            h = self._fused.get(self.unet, vae, sch, shape[0], rows, mode, self.pos_encoding, 0, program=(ts, table))
            lat = torch.empty_like(x)
            image = out if vae is not None else None
            if in_graph:
                self._fused.run_guided_rng(h, x, *noise.seed_draw_offset, z0, mask, image, latents_out=lat, check=check)
            else:
                self._fused.run_guided(h, x, zs, z0, mask, nk, nr, image, latents_out=lat, check=check)
            return lat
        if self.pos_encoding:
            pos_encoding = _pos_channel(shape[0], shape[2], shape[3], dev)
        for i, t in enumerate(self.progress_bar(ts)):
            model_input = torch.cat([x, pos_encoding], dim=1) if self.pos_encoding else x
            model_output = self.unet(model_input, t).sample
            x = guided_step(sch, table[i], model_output, x, None if zs is None else zs[i], z0, mask, None if nk is None else nk[i],
                            None if nr is None else nr[i])
        return x


class DDPMPipelineRange(_PipelineBase):
    """ldm/pipelines.py:13-117 (pixel-space ancestral sampling, no pos-encoding channel)."""

    def __init__(self, unet, scheduler):
        super().__init__()
        self.register_modules(unet=unet, scheduler=scheduler)

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, num_inference_steps=1000, output_type="torch", return_dict=True,
                 fused=True, latents=None, step_noise=None, sample_offset=0, **kwargs):
        """`latents` / `step_noise` (not in the reference signature): x_T and the [steps][B, C, W, H] ancestral noise
        already on the device, instead of drawing them from `generator`.  `sample_offset`: the first sample's index (DeviceGenerator)."""
        cfg = self.unet.config
        ss = cfg.sample_size if not isinstance(cfg.sample_size, int) else (cfg.sample_size, cfg.sample_size)
        shape = (batch_size, cfg.in_channels, *ss)
        noise = _CallNoise(generator, sample_offset, self.device)
        ancestral = isinstance(self.scheduler, DDPMSchedulerHIP)
        multistep = isinstance(self.scheduler, MultistepSchedulerBase)      # DPM-Solver++ or UniPC: no noise, fused like DDPM here
        image = None
        # (the captured loop that draws its step noise draws x_T as well when none is given: the one route with a null x_T)
        if latents is not None or not (ancestral and noise.in_graph(fused, step_noise)):
            image = noise.x_T(shape, latents, on_host=False).to(device=self.device, dtype=torch.float32)
        self.scheduler.set_timesteps(num_inference_steps)
        if fused and (ancestral or multistep):
            image = self._sample_fused(shape, image, noise, step_noise, num_inference_steps, kwargs.get("check", True))
        else:
            for i, t in enumerate(self.progress_bar(self.scheduler.timesteps)):
                model_output = self.unet(image, t).sample
                z = noise.row(1, i, shape, step_noise) if ancestral or (step_noise is not None and not multistep) else None
                kw = {"noise": z} if z is not None else {"generator": noise.torch_generator}
                image = self.scheduler.step(model_output, t, image, **kw).prev_sample
        return self._finish(image, output_type, return_dict)


class DDIMPipelineRange(_PipelineBase):
    """ldm/pipelines.py:119-258 (RangeDM: pixel-space DDIM with the pos-encoding channel)."""

    def __init__(self, unet, scheduler, pos_encoding=False):
        super().__init__()
        scheduler = DDIMSchedulerHIP.from_config(scheduler.config)      # ldm/pipelines.py:135-139
        self.register_modules(unet=unet, scheduler=scheduler)
        self.pos_encoding = pos_encoding

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, use_clipped_model_output=None,
                 output_type="torch", return_dict=True, fused=True, latents=None, known=None, known_mask=None, jump_length=1,
                 jump_n_sample=1, known_noise=None, renoise_noise=None, sample_offset=0, **kwargs):
        """`latents` (not in the reference signature): x_T already resident on the device, instead of drawing it.
        `known` (B, C, W, H normalised range image) + `known_mask` (B, 1, W, H; 1 / True = known, any pattern -- every 4th beam
        densifies): guided completion with these unconditional weights (schedulers.repaint_program; jump_length / jump_n_sample
        are RePaint's; known_noise / renoise_noise [rows, B, C, W, H] inject the draws).  The known pixels come back unchanged."""
        cfg = self.unet.config
        ss = cfg.sample_size if not isinstance(cfg.sample_size, int) else (cfg.sample_size, cfg.sample_size)
        shape = (batch_size, cfg.out_channels, *ss)
        noise = _CallNoise(generator, sample_offset, self._execution_device)
        noise.refuse_variance_noise(eta)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        image = noise.x_T(shape, latents, on_host=False).to(device=self._execution_device, dtype=self.unet.dtype)
        self.scheduler.set_timesteps(num_inference_steps)
        check = kwargs.get("check", True)
        if known is not None:
            if known_mask is None:
                raise ValueError("`known` needs `known_mask`")
            if eta != 0.0:
                raise NotImplementedError("guided DDIM sampling is eta = 0")
            m = (known_mask.to(torch.float32) > 0.5).to(torch.float32)
            image = self._guided_latents(None, image, known, m, num_inference_steps, jump_length, jump_n_sample, noise, None,
                                         known_noise, renoise_noise, fused, check)
        elif fused and eta == 0.0:
            image = self._sample_fused(shape, image, noise, None, num_inference_steps, check, pos_encoding=self.pos_encoding)
        else:
            if self.pos_encoding:
                pos_encoding = _pos_channel(shape[0], shape[2], shape[3], self.device)
            for t in self.progress_bar(self.scheduler.timesteps):
                model_input = image
                if self.pos_encoding:
                    model_input = torch.cat([model_input, pos_encoding[:model_input.shape[0]]], dim=1)
                model_output = self.unet(model_input, t).sample
                image = self.scheduler.step(model_output, t, image, eta=eta,
                                            use_clipped_model_output=use_clipped_model_output,
                                            generator=noise.torch_generator).prev_sample
        return self._finish(image, output_type, return_dict)


class LDMPipelineRange(_PipelineBase):
    """ldm/pipelines.py:261-383 (latent sampling + VAE decode).  With a DDPM scheduler this is the strided ancestral
    sampler the reference actually runs; pass a DDIMSchedulerHIP for the BASELINE's DDIM eta=0, or a
    DPMSolverMultistepSchedulerHIP for DPM-Solver++(2M) in 20-25 steps, or a UniPCMultistepSchedulerHIP for UniPC in 8-15."""

    def __init__(self, vae, unet, scheduler, pos_encoding=False):
        super().__init__()
        self.register_modules(vae=vae, unet=unet, scheduler=scheduler)
        self.pos_encoding = pos_encoding

    def _decoder_guide(self, given):
        """decoder_guidance=True: one guidance.DecoderGuide built from self.vae and kept until the VAE's weights are reloaded; a
        DecoderGuide is used as it is, unless it no longer holds this VAE's decoder."""
        from .guidance import DecoderGuide
        if isinstance(given, DecoderGuide):
            if given.stale(self.vae):
                raise ValueError("decoder_guidance was built from another VAE, or the VAE's weights were reloaded since")
            return given
        if given is not True:
            raise TypeError(f"decoder_guidance is a guidance.DecoderGuide or True, not {type(given).__name__}")
        cached = getattr(self, "_guide", None)
        if cached is None or cached.stale(self.vae):
            self._guide = cached = DecoderGuide(self.vae)
        return cached

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, output_type="torch",
                 return_dict=True, final_only=True, fused=True, latents=None, step_noise=None, known=None, known_mask=None,
                 jump_length=1, jump_n_sample=1, known_noise=None, renoise_noise=None, sample_offset=0, decoder_guidance=None,
                 guidance_scale=1.0, guidance_iters=1, guidance_start=0.0, guidance_stop=1.0, **kwargs):
        """`known` (B, 2, W, H normalised range image) + `known_mask` (B, 1, W, H pixel mask; 1 / True = known): guided completion
        with these unconditional weights.  z0 = vae.encode(known).latent_dist.mode() * scaling_factor; a latent pixel counts as
        known only if its whole footprint is (latent_known_mask), so an azimuth-span mask works and a beam-subsampling mask raises.
        step_noise / known_noise / renoise_noise are then [rows, B, C, W / f, H / f] of schedulers.repaint_program's rows.
        `return_latents=True` (guided only) returns (images, final latents, z0, latent mask).
        `decoder_guidance` (a guidance.DecoderGuide, or True to build and cache one from `self.vae`): `known` / `known_mask` take ANY
        pixel mask -- every 4th beam densifies -- and no latent replacement runs; the known pixels guide each step's clean estimate
        through the VAE decoder instead (guidance.py: DDIM with eta = 0, the eager loop; guidance_scale, guidance_iters per step,
        inside the window [guidance_start, guidance_stop) of the schedule; guidance_scale = 0 gives the bits of the unguided
        fused=False loop).  A scheduler other than DDIMSchedulerHIP, eta != 0, jump_length / jump_n_sample != 1 and final_only=False
        are refused (NotImplementedError).  `return_latents=True` then returns (images, final latents, L (B,) float64 of the last
        guided iteration); `latent_trace=` a list receives every step's latents."""
        decoder_guided = decoder_guidance is not None and decoder_guidance is not False
        if decoder_guided:
            from .guidance import decoder_guided_call, refuse_unsupported
            refuse_unsupported(self.scheduler, eta, jump_length, jump_n_sample, final_only)
        cfg = self.unet.config
        shape = (batch_size, cfg.out_channels, *cfg.sample_size)
        noise = _CallNoise(generator, sample_offset, self.device)
        latents = noise.x_T(shape, latents, on_host=True).to(self.device)
        latents = latents * self.scheduler.init_noise_sigma
        self.scheduler.set_timesteps(num_inference_steps)
        is_ddim = isinstance(self.scheduler, DDIMSchedulerHIP)
        check = kwargs.get("check", True)
        if is_ddim:
            noise.refuse_variance_noise(eta)
        if decoder_guided:
            image, lat, last = decoder_guided_call(self, self._decoder_guide(decoder_guidance), latents.float(), num_inference_steps,
                                                   known, known_mask, guidance_scale, guidance_iters, guidance_start, guidance_stop,
                                                   trace=kwargs.get("latent_trace"))
            if kwargs.get("return_latents", False):
                return image, lat, last
            return self._finish(image, output_type, return_dict)
        if known is not None:
            if known_mask is None:
                raise ValueError("`known` needs `known_mask`")
            if is_ddim and eta != 0.0:
                raise NotImplementedError("guided DDIM sampling is eta = 0")
            if not final_only:
                raise NotImplementedError("guided sampling returns the final image only")
            f = self.vae._cfg.downscale
            lat_mask = latent_known_mask(known_mask, f)
            sf = self.vae.config.scaling_factor
            z0 = self.vae.encode(known.to(self.device, torch.float32)).latent_dist.mode() * sf
            image = torch.empty((batch_size, self.vae._cfg.out_channels, shape[2] * f, shape[3] * f), device=self.device,
                                dtype=torch.float32)
            lat = self._guided_latents(self.vae, latents.float(), z0, lat_mask, num_inference_steps, jump_length, jump_n_sample,
                                       noise, step_noise, known_noise, renoise_noise, fused, check, out=image)
            if not fused:
                image = self.vae.decode(lat / sf).sample
            if kwargs.get("return_latents", False):
                return image, lat, z0, lat_mask.to(self.device)
            return self._finish(image, output_type, return_dict)
        if fused and final_only and (not is_ddim or eta == 0.0):
            image = self._sample_fused(shape, latents, noise, step_noise, num_inference_steps, check, vae=self.vae,
                                       pos_encoding=self.pos_encoding)
            return self._finish(image, output_type, return_dict)
        if not final_only:
            assert output_type == "torch"
        image_list = None if final_only else []
        pos_encoding = _pos_channel(shape[0], shape[2], shape[3], self.device) if self.pos_encoding else None
        image = self._latent_loop(latents, pos_encoding, noise, step_noise, eta, images=image_list)
        if output_type == "torch" and not final_only:
            image_list.append(image)
            return image_list
        return self._finish(image, output_type, return_dict)


class LDMUpscalePipelineRange(_PipelineBase):
    """ldm/pipelines.py:386-519 (conditional: up-sampling via a condition encoder, in-painting via masked VAE latents)."""

    def __init__(self, vae, unet, scheduler):
        super().__init__()
        self.register_modules(vae=vae, unet=unet, scheduler=scheduler)

    def encode_masked_image(self, image, mask, generator=None, noise=None):
        """ldm/pipelines.py:406-412.  `generator` / `noise` (not in the reference signature) seed or inject the draw of
        `latent_dist.sample()`."""
        image = image.to(self.unet.device)
        dist = self.vae.encode(image).latent_dist
        image = dist.sample(noise=noise) if noise is not None else dist.sample(generator=generator)
        image = image * self.vae.config.scaling_factor
        mask = mask.to(self.unet.device)
        mask = torch.nn.functional.interpolate(mask, size=image.shape[-2:])
        return torch.cat([image, mask], dim=1)

    @torch.no_grad()
    def __call__(self, image, mask=None, condition_encoder=None, batch_size=1, generator=None, eta=0.0,
                 num_inference_steps=50, output_type="torch", return_dict=True, fused=True, latents=None,
                 step_noise=None, encode_noise=None, sample_offset=0, **kwargs):
        """A DeviceGenerator gives the in-painting posterior draw (encode_noise) a draw of its own, before the sampler's."""
        if image is None:
            raise ValueError("`image` input cannot be undefined.")
        cfg = self.unet.config
        shape = (batch_size, cfg.out_channels, *cfg.sample_size)
        if mask is not None and encode_noise is None:
            encode_noise = _CallNoise.own_draw(shape, generator, sample_offset, self.unet.device)
        noise = _CallNoise(generator, sample_offset, self.unet.device)
        latents = noise.x_T(shape, latents, on_host=True).to(self.unet.device)
        if mask is None:
            assert condition_encoder is not None
            image = condition_encoder(image)
        else:
            image = self.encode_masked_image(image, mask, generator=noise.torch_generator, noise=encode_noise)
        image = image.to(dtype=latents.dtype, device=self.unet.device)
        height, width = image.shape[2:]
        assert cfg.in_channels == cfg.out_channels + image.shape[1]
        assert height == cfg.sample_size[0]
        assert width == cfg.sample_size[1]
        latents = latents * self.scheduler.init_noise_sigma
        self.scheduler.set_timesteps(num_inference_steps)
        if fused and (not isinstance(self.scheduler, DDIMSchedulerHIP) or eta == 0.0):
            out = self._sample_fused(shape, latents, noise, step_noise, num_inference_steps, kwargs.get("check", True), vae=self.vae,
                                     cond=image)
        else:
            out = self._latent_loop(latents, image, noise, step_noise, eta)
        return self._finish(out, output_type, return_dict)
