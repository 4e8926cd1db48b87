"""DDPMSchedulerHIP / DDIMSchedulerHIP -- mirror of the diffusers scheduler surface the reference touches
(SURVEY.md 8b, Appendix B): set_timesteps, timesteps, step(...).prev_sample, scale_model_input, init_noise_sigma,
add_noise, alphas_cumprod, config.  Coefficients are computed on the host in fp32 exactly as diffusers does
(torch.linspace / cumprod in float32); the elementwise update runs in librangeldm_hip.

DPMSolverMultistepSchedulerHIP -- the few-step ODE solver a diffusers user swaps in with
`DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: deterministic DPM-Solver++(2M)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .config import SchedulerConfig


class SchedulerOutput:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers.utils.torch_utils.randn_tensor semantics: a CPU generator draws on the CPU and moves.  A rng.DeviceGenerator draws
    on the device with rng.randn (fp32, one draw consumed, shape[0] the sample axis)."""
    from .rng import DeviceGenerator, StreamAddress, randn
    if isinstance(generator, (DeviceGenerator, StreamAddress)):
        x = randn(shape, generator, device=device if device is not None else "cuda")
        return x if dtype in (None, torch.float32) else x.to(dtype)
    device = torch.device(device) if device is not None else torch.device("cpu")
    rand_device = device
    if generator is not None:
        g0 = generator[0] if isinstance(generator, list) else generator
        if g0.device.type != device.type and g0.device.type == "cpu":
            rand_device = torch.device("cpu")
    if isinstance(generator, list):
        shape1 = (1,) + tuple(shape[1:])
        x = torch.cat([torch.randn(shape1, generator=g, device=rand_device, dtype=dtype) for g in generator], 0)
    else:
        x = torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype)
    return x.to(device)


# scheduler.config.prediction_type -> RLDM_PRED_* (include/rangeldm_hip.h, rldm_sched_step)
PREDICTION_TYPES = {"epsilon": 0, "v_prediction": 1, "sample": 2}


class _SchedulerBase:
    init_noise_sigma = 1.0
    order = 1
    _SPACINGS = ("leading",)

    def __init__(self, config=None, **kwargs):
        if config is None:
            config = SchedulerConfig(**kwargs)
        elif isinstance(config, dict):
            config = SchedulerConfig(**{k: v for k, v in config.items() if k in SchedulerConfig.__dataclass_fields__})
        elif not isinstance(config, SchedulerConfig):          # a SimpleNamespace / other scheduler's .config
            config = SchedulerConfig(**{k: getattr(config, k) for k in SchedulerConfig.__dataclass_fields__
                                        if hasattr(config, k)})
        c = self._cfg = config
        if c.beta_schedule != "linear" or c.timestep_spacing not in self._SPACINGS:
            raise NotImplementedError("only the reference's scheduler config is supported (linear betas, leading spacing)")
        if c.prediction_type not in PREDICTION_TYPES:
            # (the message of diffusers' schedulers; ldm/train_unconditional.py:505-510 accepts epsilon and v_prediction)
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample` or `v_prediction`")
        self.prediction_code = PREDICTION_TYPES[c.prediction_type]
        if c.clip_sample:
            raise NotImplementedError("clip_sample=True (the reference sets clip_sample=False)")
        self.config = SimpleNamespace(**c.to_dict())
        self.betas = torch.linspace(c.beta_start, c.beta_end, c.num_train_timesteps, dtype=torch.float32)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.final_alpha_cumprod = torch.tensor(1.0) if c.set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.arange(c.num_train_timesteps - 1, -1, -1, dtype=torch.int64)
        self._table_key = self._table = None

    @classmethod
    def from_config(cls, config, **kw):
        return cls(config, **kw)

    @classmethod
    def load_config(cls, path, subfolder=None):
        """`DDPMScheduler.load_config(args.scheduler_config)` (ldm/inference.py:126): json path or directory."""
        import json
        import os
        from .checkpoint import SCHEDULER_CONFIG_NAME, scheduler_config_from_diffusers
        if subfolder:
            path = os.path.join(path, subfolder)
        if os.path.isdir(path):
            path = os.path.join(path, SCHEDULER_CONFIG_NAME)
        with open(path) as f:
            return scheduler_config_from_diffusers(json.load(f))

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        return cls(cls.load_config(path, subfolder), **kw)

    def save_pretrained(self, path):
        import json
        import os
        from .checkpoint import SCHEDULER_CONFIG_NAME, scheduler_config_to_diffusers
        os.makedirs(path, exist_ok=True)
        name = "DDIMScheduler" if type(self).__name__.startswith("DDIM") else "DDPMScheduler"
        with open(os.path.join(path, SCHEDULER_CONFIG_NAME), "w") as f:
            json.dump(scheduler_config_to_diffusers(self._cfg, name), f, indent=2, sort_keys=True)

    def set_timesteps(self, num_inference_steps, device=None):
        c = self._cfg
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = c.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + c.steps_offset
        self.timesteps = torch.from_numpy(ts)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def sampler_table(self, eta=0.0):
        """[steps][5] fp32 coefficient rows of the current timesteps (rldm_sampler_config::coef), memoised per schedule."""
        key = (self.timesteps.numpy().tobytes(), float(eta))
        if self._table_key != key:
            rows = [self._sampler_row(int(t), eta) for t in self.timesteps]
            self._table = np.ascontiguousarray(np.asarray(rows, dtype=np.float32).reshape(-1, 5))
            self._table_key = key
        return self._table

    def _prev_t(self, t):
        n = self.num_inference_steps or self._cfg.num_train_timesteps
        return t - self._cfg.num_train_timesteps // n

    def _alphas(self, t):
        prev_t = self._prev_t(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self._alpha_final()
        return a_t, a_prev

    def _noised(self, first, second, timesteps, sign, what):
        """sqrt(abar_t) * first + sign * sqrt(1 - abar_t) * second per sample (rldm_sched_add_noise); `first` gives device and shape."""
        a = self.alphas_cumprod[timesteps.detach().to("cpu", torch.int64).reshape(-1)]
        sa = (a ** 0.5).numpy().astype(np.float32)
        sb = (sign * (1 - a) ** 0.5).numpy().astype(np.float32)
        B = first.shape[0]
        out = torch.empty_like(first)
        _lib.check(_lib.lib().rldm_sched_add_noise(
            _lib.ptr(first), _lib.ptr(second), sa.ctypes.data_as(C.POINTER(C.c_float)), sb.ctypes.data_as(C.POINTER(C.c_float)), B,
            first.numel() // B, _lib.ptr(out), _lib.stream_ptr(first.device)), what)
        return out

    def add_noise(self, original_samples, noise, timesteps):
        x0 = original_samples.to(dtype=torch.float32).contiguous()
        nz = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        return self._noised(x0, nz, timesteps, 1.0, "rldm_sched_add_noise")

    def get_velocity(self, sample, noise, timesteps):
        """`DDPMScheduler.get_velocity` (the v_prediction target, ldm/train_unconditional.py:507-508):
        v = sqrt(alpha_prod_t) * noise - sqrt(1 - alpha_prod_t) * sample.  The same elementwise map as add_noise with the two
        tensors swapped and the second coefficient negated."""
        x0 = sample.to(dtype=torch.float32).contiguous()
        nz = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        return self._noised(nz, x0, timesteps, -1.0, "rldm_sched_add_noise (get_velocity)")

    def _launch(self, sampler_mode, coef, model_output, sample, noise):
        e = model_output.to(dtype=torch.float32).contiguous()
        x = sample.to(device=e.device, dtype=torch.float32).contiguous()
        nz = None if noise is None else noise.to(device=e.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        cf = (C.c_float * 5)(*[float(v) for v in coef])
        _lib.check(_lib.lib().rldm_sched_step(sampler_mode, self.prediction_code, cf, _lib.ptr(e), _lib.ptr(x), _lib.ptr(nz), _lib.ptr(out),
                                              x.numel(), _lib.stream_ptr(e.device)), "scheduler step")
        return out


class DDPMSchedulerHIP(_SchedulerBase):
    """Strided ancestral DDPM, variance_type fixed_small (what `LDMPipelineRange` runs as shipped)."""

    def _alpha_final(self):
        return self.one

    def coefficients(self, t):
        t = int(t)
        a_t, a_prev = self._alphas(t)
        b_t, b_prev = 1 - a_t, 1 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1 - cur_a
        sigma = torch.clamp(b_prev / b_t * cur_b, min=1e-20) ** 0.5 if t > 0 else torch.tensor(0.0)
        return [float(a_t ** 0.5), float(b_t ** 0.5), float((a_prev ** 0.5 * cur_b) / b_t),
                float(cur_a ** 0.5 * b_prev / b_t), float(sigma)]

    def _sampler_row(self, t, eta):
        return self.coefficients(t)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        coef = self.coefficients(timestep)
        if coef[4] != 0.0 and noise is None:
            noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                 dtype=torch.float32)
        prev = self._launch(1, coef, model_output, sample, noise if coef[4] != 0.0 else None)
        return SchedulerOutput(prev) if return_dict else (prev,)


class DDIMSchedulerHIP(_SchedulerBase):
    def _alpha_final(self):
        return self.final_alpha_cumprod

    def coefficients(self, t, eta=0.0):
        t = int(t)
        a_t, a_prev = self._alphas(t)
        b_t, b_prev = 1 - a_t, 1 - a_prev
        var = (b_prev / b_t) * (1 - a_t / a_prev)
        std = eta * var ** 0.5
        return [float(a_t ** 0.5), float(b_t ** 0.5), float(a_prev ** 0.5), float((1 - a_prev - std ** 2) ** 0.5),
                float(std)]

    def _sampler_row(self, t, eta):
        return self.coefficients(t, eta)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        coef = self.coefficients(timestep, eta)
        noise = variance_noise
        if coef[4] != 0.0 and noise is None:
            noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                 dtype=torch.float32)
        prev = self._launch(0, coef, model_output, sample, noise if coef[4] != 0.0 else None)
        return SchedulerOutput(prev) if return_dict else (prev,)


# DPMSolverMultistepScheduler settings: the supported value of each (diffusers' names); any other value raises
_DPM_FIXED = {"algorithm_type": "dpmsolver++", "solver_type": "midpoint", "lower_order_final": True, "euler_at_final": False,
              "final_sigmas_type": "zero", "use_karras_sigmas": False, "thresholding": False}
_DPM_KEYS = tuple(_DPM_FIXED) + ("solver_order", "lambda_min_clipped")


def _config_items(config):
    if config is None:
        return {}
    if isinstance(config, dict):
        return dict(config)
    if isinstance(config, SchedulerConfig):
        return config.to_dict()
    return dict(vars(config))                          # a SimpleNamespace: another scheduler's .config


class DPMSolverMultistepSchedulerHIP(_SchedulerBase):
    """diffusers DPMSolverMultistepScheduler with algorithm_type="dpmsolver++", solver_type="midpoint", solver_order 1 or 2,
    lower_order_final=True, euler_at_final=False, final_sigmas_type="zero", no Karras sigmas, no thresholding,
    lambda_min_clipped=-inf: deterministic DPM-Solver++(2M), for the three prediction types.

    Every step is prev = c_x0 * x0 + c_xt * x + c_x0prev * x0_prev, one row [alpha_i, s_i, c_x0, c_xt, c_x0prev] per step
    (include/rangeldm_hip.h, rldm_sched_dpmsolver_step), computed on the host in float64 from the fp32 alphas_cumprod and stored
    as fp32.  `step` keeps the step index and the previous x0 (a device tensor); set_timesteps resets both.  The captured
    sampler (RLDM_SAMPLER_DPMSOLVER) runs the same rows with the history on the device."""

    _SPACINGS = ("leading", "linspace", "trailing")

    def __init__(self, config=None, **kwargs):
        d = _config_items(config)
        d.update(kwargs)
        solver = {"solver_order": 2, "lambda_min_clipped": -math.inf, **_DPM_FIXED}
        solver.update({k: d[k] for k in _DPM_KEYS if k in d})
        for k, want in _DPM_FIXED.items():
            if solver[k] != want:
                raise NotImplementedError(f"DPMSolverMultistepScheduler {k}={solver[k]!r}: only {want!r} is implemented")
        if solver["solver_order"] not in (1, 2):
            raise NotImplementedError(f"DPMSolverMultistepScheduler solver_order={solver['solver_order']!r}: only 1 and 2 are implemented")
        if solver["lambda_min_clipped"] != -math.inf:
            raise NotImplementedError(f"DPMSolverMultistepScheduler lambda_min_clipped={solver['lambda_min_clipped']!r}: only -inf is implemented")
        spacing = d.get("timestep_spacing", "leading")
        if spacing not in self._SPACINGS:
            raise NotImplementedError(f"DPMSolverMultistepScheduler timestep_spacing={spacing!r}: only {self._SPACINGS} are implemented")
        # clip_sample / variance_type / set_alpha_to_one of a DDPM / DDIM config mean nothing to this solver (diffusers ignores them)
        base = {k: d[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type",
                                  "timestep_spacing", "steps_offset") if k in d}
        if base.get("beta_schedule", "linear") != "linear":
            raise NotImplementedError(f"DPMSolverMultistepScheduler beta_schedule={base['beta_schedule']!r}: only 'linear' is implemented")
        super().__init__(SchedulerConfig(**base))
        self.solver_order = int(solver["solver_order"])
        self._solver = solver
        self.config = SimpleNamespace(**{k: v for k, v in self._cfg.to_dict().items()
                                         if k not in ("clip_sample", "variance_type", "set_alpha_to_one")}, **solver)
        self.sigmas = None
        self._schedules = {}
        self._reset()

    def _reset(self):
        self._step_index = None
        self._hist = None
        self._have_x0 = False

    @property
    def step_index(self):
        return self._step_index

    @classmethod
    def load_config(cls, path, subfolder=None):
        import json
        import os
        from .checkpoint import SCHEDULER_CONFIG_NAME
        if subfolder:
            path = os.path.join(path, subfolder)
        if os.path.isdir(path):
            path = os.path.join(path, SCHEDULER_CONFIG_NAME)
        with open(path) as f:
            d = json.load(f)
        return {k: v for k, v in d.items() if not k.startswith("_")}

    def save_pretrained(self, path):
        import json
        import os
        from .checkpoint import SCHEDULER_CONFIG_NAME
        os.makedirs(path, exist_ok=True)
        d = {"_class_name": "DPMSolverMultistepScheduler", "_diffusers_version": "0.21.0"}
        d.update(vars(self.config))
        with open(os.path.join(path, SCHEDULER_CONFIG_NAME), "w") as f:
            json.dump(d, f, indent=2, sort_keys=True)          # (lambda_min_clipped: -Infinity, as diffusers writes it)

    def _timesteps(self, n):
        c = self._cfg
        T = c.num_train_timesteps
        if c.timestep_spacing == "leading":
            r = T // (n + 1)
            ts = (np.arange(0, n + 1) * r).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        else:
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1
        if len(ts) != n or ts.min() < 0 or ts.max() >= T or (n > 1 and np.any(np.diff(ts) >= 0)):
            raise ValueError(f"{n} inference steps with timestep_spacing={c.timestep_spacing!r} do not give {n} distinct timesteps "
                             f"in [0, {T})")
        return ts

    def _rows(self, ts, order):
        """[N][5] float64 rows [alpha_i, s_i, c_x0, c_xt, c_x0prev] (the class docstring)."""
        ac = self.alphas_cumprod.numpy().astype(np.float64)[ts]
        n = len(ts)
        sigma = np.sqrt((1.0 - ac) / ac)
        alpha = 1.0 / np.sqrt(sigma ** 2 + 1.0)
        s = sigma * alpha
        lam = np.log(alpha) - np.log(s)
        rows = np.zeros((n, 5), dtype=np.float64)
        rows[:, 0], rows[:, 1] = alpha, s
        for i in range(n):
            if i == n - 1:                                  # sigma_N = 0: first order, phi = -1, the step returns x0
                rows[i, 2:] = (1.0, 0.0, 0.0)
                continue
            h = lam[i + 1] - lam[i]
            phi = math.exp(-h) - 1.0
            rows[i, 3] = s[i + 1] / s[i]
            if i == 0 or order == 1:
                rows[i, 2] = -alpha[i + 1] * phi
            else:
                r = (lam[i] - lam[i - 1]) / h
                rows[i, 2] = -alpha[i + 1] * phi * (1.0 + 1.0 / (2.0 * r))
                rows[i, 4] = alpha[i + 1] * phi / (2.0 * r)
        return rows

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps < 1 or num_inference_steps > self._cfg.num_train_timesteps:
            raise ValueError("num_inference_steps must be in [1, num_train_timesteps]")
        if num_inference_steps not in self._schedules:      # (the pipelines set the timesteps on every call: computed once)
            ts = self._timesteps(num_inference_steps)
            ac = self.alphas_cumprod.numpy().astype(np.float64)[ts]
            sigmas = torch.from_numpy(np.concatenate([np.sqrt((1.0 - ac) / ac), [0.0]]).astype(np.float32))
            self._schedules[num_inference_steps] = (ts, sigmas, np.ascontiguousarray(self._rows(ts, self.solver_order).astype(np.float32)),
                                                    np.ascontiguousarray(self._rows(ts, 1).astype(np.float32)))
        ts, self.sigmas, self._table, self._table_first = self._schedules[num_inference_steps]
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts.copy())
        self._reset()

    def coefficients(self):
        """The [num_inference_steps][5] fp32 rows of the current timesteps (rldm_sampler_config::coef, RLDM_SAMPLER_DPMSOLVER)."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        return self._table

    def sampler_table(self, eta=0.0):
        return self.coefficients()

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        if self._step_index is None:
            hit = (self.timesteps == int(timestep)).nonzero()
            if len(hit) == 0:
                raise ValueError(f"timestep {int(timestep)} is not in scheduler.timesteps")
            self._step_index = int(hit[0, 0])
        i = self._step_index
        if i >= self.num_inference_steps:
            raise ValueError("step called more often than num_inference_steps after set_timesteps")
        e = model_output.to(dtype=torch.float32).contiguous()
        x = sample.to(device=e.device, dtype=torch.float32).contiguous()
        if self._hist is None or self._hist.shape != x.shape or self._hist.device != x.device:
            self._hist = torch.empty_like(x)
            self._have_x0 = False
        # without a previous x0 (the first step taken since set_timesteps) the step is first order, as diffusers' lower_order_nums
        row = self._table[i] if self._have_x0 else self._table_first[i]
        out = torch.empty_like(x)
        cf = (C.c_float * 5)(*[float(v) for v in row])
        _lib.check(_lib.lib().rldm_sched_dpmsolver_step(self.prediction_code, cf, _lib.ptr(e), _lib.ptr(x), _lib.ptr(self._hist), _lib.ptr(out),
                                                        x.numel(), _lib.stream_ptr(e.device)), "DPM-Solver++ step")
        self._have_x0 = True
        self._step_index = i + 1
        return SchedulerOutput(out) if return_dict else (out,)


def sampler_mode(scheduler):
    """rldm_sampler_config::mode of a scheduler: DDIM, DPM-Solver++, else the (strided ancestral) DDPM step."""
    if isinstance(scheduler, DDIMSchedulerHIP):
        return _lib.RLDM_SAMPLER_DDIM
    if isinstance(scheduler, DPMSolverMultistepSchedulerHIP):
        return _lib.RLDM_SAMPLER_DPMSOLVER
    return _lib.RLDM_SAMPLER_DDPM


# ---- guided sampling on unconditional weights (RePaint-style known-region replacement) -----------------------------------
def repaint_program(scheduler, num_inference_steps, jump_length=1, jump_n_sample=1):
    """The row program of a guided sampler: (timesteps int64 [rows], table fp32 [rows][9]).

    Let N = num_inference_steps and "remaining" the number of denoise steps still needed to reach the clean sample.  A row
    denoises from remaining m + 1 to m with the scheduler's own step (columns 0-4: its `sampler_table` row of that timestep),
    replaces the known region by the observation noised to the level the row ends at (columns 5-6: ka, kb = sqrt(a_prev),
    sqrt(1 - a_prev), with the a_prev the scheduler itself uses -- 1 after the last timestep) and, when m - 1 is a non-negative
    multiple of jump_length below N - jump_length that has been reached fewer than jump_n_sample times, re-noises up to remaining
    m + jump_length (columns 7-8: ra, rb = sqrt(a_hi / a_lo), sqrt(1 - a_hi / a_lo); (1, 0) otherwise).  This is RePaint's
    jump schedule (Lugmayr et al. 2022); with jump_n_sample = 1 the program is the scheduler's N timesteps.
    rows = N + (jump_n_sample - 1) * jump_length * (number of jump points)."""
    if isinstance(scheduler, DPMSolverMultistepSchedulerHIP):
        raise NotImplementedError("guided sampling runs DDPM or DDIM (eta = 0) rows: DPM-Solver++ keeps an x0 history that means "
                                  "nothing across a jump back up")
    N, jl, jn = int(num_inference_steps), int(jump_length), int(jump_n_sample)
    if N < 1 or jl < 1 or jn < 1:
        raise ValueError("num_inference_steps, jump_length and jump_n_sample must be >= 1")
    scheduler.set_timesteps(N)
    ts = [int(t) for t in scheduler.timesteps]
    ac = scheduler.alphas_cumprod.numpy().astype(np.float64)
    visits = {}
    out_t, rows = [], []
    rem = N
    while rem >= 1:
        t = ts[N - rem]
        m = rem - 1
        row = [float(v) for v in np.asarray(scheduler._sampler_row(t, 0.0), dtype=np.float32)]
        a_lo = float(scheduler._alphas(t)[1])               # the level this row ends at, before any re-noise
        ra, rb = 1.0, 0.0
        p = m - 1
        if p >= 0 and p % jl == 0 and p < N - jl:
            visits[p] = visits.get(p, 0) + 1
            if visits[p] < jn:
                a_hi = ac[ts[N - (m + jl)]]
                ra, rb = math.sqrt(a_hi / a_lo), math.sqrt(1.0 - a_hi / a_lo)
                m += jl
        out_t.append(t)
        rows.append(row + [math.sqrt(a_lo), math.sqrt(1.0 - a_lo), ra, rb])
        rem = m
    return (torch.tensor(out_t, dtype=torch.int64),
            np.ascontiguousarray(np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(-1, 9)))


def guided_step(scheduler, row, model_output, sample, noise, known, mask, known_noise, renoise_noise):
    """One row of a guided program outside the captured loop (rldm_sched_guided_step): the scheduler's step with row[0:5], the
    known-region blend with row[5:7], the re-noise with row[7:9].  mask: [B, 1, W, H], 1 = known."""
    mode = sampler_mode(scheduler)
    if mode == _lib.RLDM_SAMPLER_DPMSOLVER:
        raise NotImplementedError("guided sampling runs DDPM or DDIM (eta = 0) rows")
    e = model_output.to(dtype=torch.float32).contiguous()
    ptr = _lib.ptr

    def dev(t):
        return None if t is None else t.to(device=e.device, dtype=torch.float32).contiguous()
    x, z0, m = dev(sample), dev(known), dev(mask)
    nz = dev(noise) if row[4] != 0.0 else None
    nk = dev(known_noise) if row[6] != 0.0 else None
    nr = dev(renoise_noise) if (row[7] != 1.0 or row[8] != 0.0) else None
    B, Cc = x.shape[0], x.shape[1]
    spatial = x.numel() // (B * Cc)
    if z0.shape != x.shape or m.numel() != B * spatial:
        raise ValueError(f"known {tuple(z0.shape)} / mask {tuple(m.shape)} do not match the sample {tuple(x.shape)}")
    out = torch.empty_like(x)
    cf = (C.c_float * 9)(*[float(v) for v in row])
    _lib.check(_lib.lib().rldm_sched_guided_step(mode, scheduler.prediction_code, cf, ptr(e), ptr(x), ptr(nz), ptr(z0), ptr(m), ptr(nk),
                                                 ptr(nr), ptr(out), B, Cc, spatial, _lib.stream_ptr(e.device)), "guided scheduler step")
    return out
