"""DDPMSchedulerHIP / DDIMSchedulerHIP -- mirror of the diffusers scheduler surface the reference touches
(SURVEY.md 8b, Appendix B): set_timesteps, timesteps, step(...).prev_sample, scale_model_input, init_noise_sigma,
add_noise, alphas_cumprod, config.  Coefficients are computed on the host in fp32 exactly as diffusers does
(torch.linspace / cumprod in float32); the elementwise update runs in librangeldm_hip.

DPMSolverMultistepSchedulerHIP -- the few-step ODE solver a diffusers user swaps in with
`DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: deterministic DPM-Solver++(2M).
UniPCMultistepSchedulerHIP -- diffusers' UniPCMultistepScheduler (bh2, data prediction): a predictor of order up to 3 and a corrector
that costs no network evaluation, for 8-15 steps."""
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


class MultistepSchedulerBase(_SchedulerBase):
    """What the multistep ODE solvers share: the three timestep spacings, the grid (alpha_i, s_i, lambda_i) in float64 from the fp32
    alphas_cumprod, a step index, a table of per-step rows made by
    set_timesteps, and a config file that carries the solver's own settings.  A subclass gives _DIFFUSERS_NAME, _rows, set_timesteps, _reset and step."""

    _SPACINGS = ("leading", "linspace", "trailing")
    _DIFFUSERS_NAME = None

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
        d = {"_class_name": self._DIFFUSERS_NAME, "_diffusers_version": "0.21.0"}
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

    def _grid(self, ts):
        """(alpha, s, lambda), float64 [N + 1]: at the N timesteps and behind the last one (alpha = 1, s = 0, lambda = +inf)."""
        ac = self.alphas_cumprod.numpy().astype(np.float64)[ts]
        sigma = np.append(np.sqrt((1.0 - ac) / ac), 0.0)
        alpha = 1.0 / np.sqrt(sigma ** 2 + 1.0)
        s = sigma * alpha
        with np.errstate(divide="ignore"):
            lam = np.log(alpha) - np.log(s)
        return alpha, s, lam

    def coefficients(self):
        """The fp32 rows of the current timesteps, one per step (rldm_sampler_config::coef of the solver's sampler mode)."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        return self._table

    def sampler_table(self, eta=0.0):
        return self.coefficients()


class DPMSolverMultistepSchedulerHIP(MultistepSchedulerBase):
    """diffusers DPMSolverMultistepScheduler with algorithm_type="dpmsolver++", solver_type="midpoint", solver_order 1 or 2,
    lower_order_final=True, euler_at_final=False, final_sigmas_type="zero", no Karras sigmas, no thresholding,
    lambda_min_clipped=-inf: deterministic DPM-Solver++(2M), for the three prediction types.

    Every step is prev = c_x0 * x0 + c_xt * x + c_x0prev * x0_prev, one row [alpha_i, s_i, c_x0, c_xt, c_x0prev] per step
    (include/rangeldm_hip.h, rldm_sched_dpmsolver_step), computed on the host in float64 from the fp32 alphas_cumprod and stored
    as fp32.  `step` keeps the step index and the previous x0 (a device tensor); set_timesteps resets both.  The captured
    sampler (RLDM_SAMPLER_DPMSOLVER) runs the same rows with the history on the device."""

    _DIFFUSERS_NAME = "DPMSolverMultistepScheduler"

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

    def _rows(self, ts, order):
        """[N][5] float64 rows [alpha_i, s_i, c_x0, c_xt, c_x0prev] (the class docstring)."""
        n = len(ts)
        alpha, s, lam = self._grid(ts)                      # (the entries behind the last timestep are not used: the last row is fixed)
        rows = np.zeros((n, 5), dtype=np.float64)
        rows[:, 0], rows[:, 1] = alpha[:n], s[:n]
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


# UniPCMultistepScheduler settings: the supported value of each (diffusers' names); any other value raises
_UNIPC_FIXED = {"solver_type": "bh2", "predict_x0": True, "lower_order_final": True, "final_sigmas_type": "zero",
                "use_karras_sigmas": False, "thresholding": False, "solver_p": None}
_UNIPC_KEYS = tuple(_UNIPC_FIXED) + ("solver_order", "disable_corrector")


class UniPCMultistepSchedulerHIP(MultistepSchedulerBase):
    """diffusers UniPCMultistepScheduler with solver_type="bh2" (B(h) = e^h - 1), predict_x0=True, solver_order 1, 2 or 3,
    lower_order_final=True, final_sigmas_type="zero", no Karras sigmas, no thresholding, no solver_p: the predictor UniP-p and the
    corrector UniC-p of Zhao et al. 2023 in data-prediction form, for the three prediction types.  It shares DPM-Solver++'s grid
    (timesteps, alpha_i, s_i, lambda_i: the parent class), and UniP-2 without the corrector is DPM-Solver++(2M).

    Step i runs with order o_i = min(solver_order, N - i, steps taken so far + 1).  m_i is the x0 prediction converted from the model
    output with the sample the network saw.  At i >= 1 (unless i - 1 is in disable_corrector) the corrector UniC of order o_{i-1}
    first replaces that sample x_i by x_c, recomputed from the previous step's corrected sample `last` with m_i as the extra node;
    then the predictor UniP-o_i goes from x_c to x_{i+1}.  Every term is linear in the tensors, so a step is one row

        [alpha_i, s_i, use_corr, k_last, k_1, k_2, k_3, k_t, p_x, p_0, p_1, p_2]
        x_c    = k_last * last + k_1 * m_{i-1} + k_2 * m_{i-2} + k_3 * m_{i-3} + k_t * m_i         (use_corr; else x_c = x_i)
        x_next = p_x * x_c + p_0 * m_i + p_1 * m_{i-1} + p_2 * m_{i-2}

    (include/rangeldm_hip.h, rldm_sched_unipc_step), computed on the host in float64 and stored as fp32; a coefficient the step does
    not use is exactly 0 and its tensor is not read.  `step` keeps the step index, `last` and the three latest m on the device;
    set_timesteps resets them.  A `step` sequence that starts behind the first timestep warms its order up from there (its rows are
    then computed at the call: diffusers' lower_order_nums counts steps, not indices).

    solver_type "midpoint", "heun" and "logrho" -- another solver's setting, which `from_config(dpm_scheduler.config)` carries -- become
    "bh2", as diffusers' own constructor does; every other solver_type but "bh2" raises.  The captured sampler (RLDM_SAMPLER_UNIPC) runs the same rows with that state per lane."""

    _DIFFUSERS_NAME = "UniPCMultistepScheduler"

    def __init__(self, config=None, **kwargs):
        d = _config_items(config)
        d.update(kwargs)
        solver = {"solver_order": 2, "disable_corrector": [], **_UNIPC_FIXED}
        solver.update({k: d[k] for k in _UNIPC_KEYS if k in d})
        if solver["solver_type"] in ("midpoint", "heun", "logrho"):       # another solver's config: diffusers falls back to bh2 as well
            solver["solver_type"] = "bh2"
        for k, want in _UNIPC_FIXED.items():
            if solver[k] is not want and solver[k] != want:
                raise NotImplementedError(f"UniPCMultistepScheduler {k}={solver[k]!r}: only {want!r} is implemented")
        if solver["solver_order"] not in (1, 2, 3):
            raise NotImplementedError(f"UniPCMultistepScheduler solver_order={solver['solver_order']!r}: only 1, 2 and 3 are implemented")
        solver["disable_corrector"] = sorted(int(i) for i in solver["disable_corrector"])
        spacing = d.get("timestep_spacing", "leading")
        if spacing not in self._SPACINGS:
            raise NotImplementedError(f"UniPCMultistepScheduler timestep_spacing={spacing!r}: only {self._SPACINGS} are implemented")
        base = {k: d[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type",
                                  "timestep_spacing", "steps_offset") if k in d}
        if base.get("beta_schedule", "linear") != "linear":
            raise NotImplementedError(f"UniPCMultistepScheduler beta_schedule={base['beta_schedule']!r}: only 'linear' is implemented")
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
        self._taken = 0                                     # steps since set_timesteps: diffusers' lower_order_nums, not capped
        self._last = self._hist = None

    def _update(self, grid, j, t, order, corrector):
        """One UniP / UniC update of order `order` from grid index j to t as coefficients (c_x, c_m, [c_1, c_2], c_t) of the sample at j,
        m_j, m_{j-1}, m_{j-2} and (corrector) m_t."""
        alpha, s, lam = grid
        if s[t] == 0.0:                                     # sigma_N = 0: phi1 = -1 and the order is 1, the step returns m_j
            return 0.0, 1.0, [0.0, 0.0], 0.0
        h = lam[t] - lam[j]
        hh = -h
        phi1 = B = math.expm1(hh)
        rks = [(lam[j - k] - lam[j]) / h for k in range(1, order)]
        n_rho = order if corrector else order - 1
        if n_rho <= 1:
            rho = [0.5] * n_rho                             # (diffusers' constants for UniP-2 and UniC-1)
        else:
            nodes = (rks + [1.0])[:n_rho]
            R = np.asarray([[r ** jj for r in nodes] for jj in range(n_rho)], dtype=np.float64)
            b, hphi, fact = [], phi1 / hh - 1.0, 1.0
            for jj in range(1, n_rho + 1):
                b.append(hphi * fact / B)
                fact *= jj + 1
                hphi = hphi / hh - 1.0 / fact
            rho = [float(v) for v in np.linalg.solve(R, np.asarray(b, dtype=np.float64))]
        g = alpha[t] * B
        older = [-g * rho[k] / rks[k] for k in range(order - 1)]
        c_t = -g * rho[order - 1] if corrector else 0.0
        return s[t] / s[j], -alpha[t] * phi1 - sum(older) - c_t, (older + [0.0, 0.0])[:2], c_t

    def _row(self, grid, i, taken):
        """The float64 row of step i when `taken` steps came before it since set_timesteps (the table: taken = i)."""
        n = len(grid[0]) - 1
        row = np.zeros(12, dtype=np.float64)
        row[0], row[1] = grid[0][i], grid[1][i]
        if taken >= 1 and (i - 1) not in self._solver["disable_corrector"]:
            c_x, c_m, older, c_t = self._update(grid, i - 1, i, min(self.solver_order, n - i + 1, taken), True)
            row[2:8] = (1.0, c_x, c_m, older[0], older[1], c_t)
        c_x, c_m, older, _ = self._update(grid, i, i + 1, min(self.solver_order, n - i, taken + 1), False)
        row[8:12] = (c_x, c_m, older[0], older[1])
        return row

    def _rows(self, ts):
        """[N][12] float64 rows (the class docstring)."""
        grid = self._grid(ts)
        return np.asarray([self._row(grid, i, i) for i in range(len(ts))], dtype=np.float64).reshape(-1, 12)

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps < 1 or num_inference_steps > self._cfg.num_train_timesteps:
            raise ValueError("num_inference_steps must be in [1, num_train_timesteps]")
        if num_inference_steps not in self._schedules:
            ts = self._timesteps(num_inference_steps)
            grid = self._grid(ts)
            sigmas = torch.from_numpy((grid[1] / grid[0]).astype(np.float32))
            self._schedules[num_inference_steps] = (ts, sigmas, np.ascontiguousarray(self._rows(ts).astype(np.float32)), grid)
        ts, self.sigmas, self._table, self._grid_now = self._schedules[num_inference_steps]
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts.copy())
        self._reset()

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
        if self._last is None or self._last.shape != x.shape or self._last.device != x.device:
            self._last = torch.empty_like(x)
            self._hist = torch.empty((3, *x.shape), device=x.device, dtype=torch.float32)
            self._taken = 0
        # a run that starts behind the first timestep warms its order up from there, as diffusers' lower_order_nums does
        row = self._table[i] if self._taken == i else self._row(self._grid_now, i, self._taken).astype(np.float32)
        out = torch.empty_like(x)
        cf = (C.c_float * 12)(*[float(v) for v in row])
        _lib.check(_lib.lib().rldm_sched_unipc_step(self.prediction_code, cf, _lib.ptr(e), _lib.ptr(x), _lib.ptr(self._last),
                                                    _lib.ptr(self._hist), _lib.ptr(out), x.numel(), _lib.stream_ptr(e.device)), "UniPC step")
        self._taken += 1
        self._step_index = i + 1
        return SchedulerOutput(out) if return_dict else (out,)


def sampler_mode(scheduler):
    """rldm_sampler_config::mode of a scheduler: DDIM, UniPC, DPM-Solver++, else the (strided ancestral) DDPM step."""
    if isinstance(scheduler, DDIMSchedulerHIP):
        return _lib.RLDM_SAMPLER_DDIM
    if isinstance(scheduler, UniPCMultistepSchedulerHIP):
        return _lib.RLDM_SAMPLER_UNIPC
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
    if isinstance(scheduler, MultistepSchedulerBase):
        raise NotImplementedError("guided sampling runs DDPM or DDIM (eta = 0) rows: DPM-Solver++ and UniPC keep an x0 history that means "
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
    if mode in (_lib.RLDM_SAMPLER_DPMSOLVER, _lib.RLDM_SAMPLER_UNIPC):
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
