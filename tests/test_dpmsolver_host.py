"""CPU: DPMSolverMultistepSchedulerHIP's host side -- timesteps, sigmas and the coefficient rows against a float64 restatement of
diffusers' DPMSolverMultistepScheduler (dpmsolver++, midpoint, lower_order_final, final_sigmas_type "zero"), the solver's accuracy on
a data distribution whose probability-flow ODE is known in closed form, and the config surface."""
import json
import math
import os

import numpy as np
import pytest
import torch

from rangeldm_amd.config import SchedulerConfig
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP

T_TRAIN = 1000
STEP_COUNTS = (1, 5, 10, 20, 25, 50)
SPACINGS = ("leading", "linspace", "trailing")


# ---- the restatement (float64 from the fp32 alphas_cumprod) -------------------------------------------------------------
def alphas_cumprod():
    betas = torch.linspace(1e-4, 0.02, T_TRAIN, dtype=torch.float32)
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


def ref_timesteps(n, spacing, offset=0):
    if spacing == "leading":
        r = T_TRAIN // (n + 1)
        return (np.arange(n + 1) * r)[::-1][:-1] + offset
    if spacing == "linspace":
        return np.round(np.linspace(0, T_TRAIN - 1, n + 1))[::-1][:-1].astype(np.int64)
    return (np.round(np.arange(T_TRAIN, 0, -T_TRAIN / n)) - 1).astype(np.int64)


def ref_rows(ts, order=2):
    ac = alphas_cumprod()[ts]
    sig = np.append(np.sqrt((1 - ac) / ac), 0.0)
    alpha = 1 / np.sqrt(sig ** 2 + 1)
    s = sig * alpha
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(s)                     # lambda_N = +inf
    n = len(ts)
    rows = []
    for i in range(n):
        h = lam[i + 1] - lam[i]
        phi = np.exp(-h) - 1                                # -1 at the last step
        c_xt = s[i + 1] / s[i]
        if i == 0 or order == 1 or i == n - 1:
            rows.append([alpha[i], s[i], -alpha[i + 1] * phi, c_xt, 0.0])
        else:
            r = (lam[i] - lam[i - 1]) / h
            rows.append([alpha[i], s[i], -alpha[i + 1] * phi * (1 + 1 / (2 * r)), c_xt, alpha[i + 1] * phi / (2 * r)])
    return np.asarray(rows), sig


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", STEP_COUNTS)
def test_timesteps_sigmas_and_rows_match_restatement(n, spacing):
    sch = DPMSolverMultistepSchedulerHIP(timestep_spacing=spacing)
    sch.set_timesteps(n)
    ts = ref_timesteps(n, spacing)
    assert sch.timesteps.dtype == torch.int64
    assert np.array_equal(sch.timesteps.numpy(), ts)
    rows, sig = ref_rows(ts)
    np.testing.assert_allclose(sch.sigmas.numpy().astype(np.float64), sig, rtol=1e-6, atol=0)
    tab = sch.coefficients()
    assert tab.dtype == np.float32 and tab.shape == (n, 5)
    np.testing.assert_allclose(tab.astype(np.float64), rows, rtol=1e-6, atol=0)
    assert tab[0, 4] == 0.0                                  # first step: first order
    assert list(tab[-1, 2:]) == [1.0, 0.0, 0.0]              # last step: returns x0
    if n > 2:
        assert np.all(tab[1:-1, 4] != 0.0)                   # second order in between
    first = DPMSolverMultistepSchedulerHIP(timestep_spacing=spacing, solver_order=1)
    first.set_timesteps(n)
    rows1, _ = ref_rows(ts, order=1)
    assert np.all(first.coefficients()[:, 4] == 0.0)
    np.testing.assert_allclose(first.coefficients().astype(np.float64), rows1, rtol=1e-6, atol=0)


def test_documented_timesteps():
    sch = DPMSolverMultistepSchedulerHIP()                      # the reference's config: leading spacing
    sch.set_timesteps(20)
    assert sch.timesteps[:3].tolist() == [940, 893, 846] and sch.timesteps[-1] == 47
    tr = DPMSolverMultistepSchedulerHIP(timestep_spacing="trailing")
    tr.set_timesteps(20)
    assert tr.timesteps[:3].tolist() == [999, 949, 899] and tr.timesteps[-1] == 49
    assert sch.init_noise_sigma == 1.0
    x = torch.randn(2, 3)
    assert sch.scale_model_input(x, 940) is x


# ---- accuracy: Gaussian data, exact epsilon, exact probability-flow ODE solution ---------------------------------------
MU, SD = 0.5, 0.8


def exact_eps(x, a, s):
    return s * (x - a * MU) / (a * a * SD * SD + s * s)


def run_dpm(rows, x):
    x0_prev = np.zeros_like(x)
    for a, s, c_x0, c_xt, c_x0p in rows.astype(np.float64):
        x0 = (x - s * exact_eps(x, a, s)) / a
        x, x0_prev = c_x0 * x0 + c_xt * x + c_x0p * x0_prev, x0
    return x


def run_ddim(rows, x):
    for a, s, c_x0, c_dir, _ in rows.astype(np.float64):
        e = exact_eps(x, a, s)
        x = c_x0 * (x - s * e) / a + c_dir * e
    return x


def ode_target(x_T, a0, s0):
    return MU + SD * (x_T - a0 * MU) / math.sqrt(a0 * a0 * SD * SD + s0 * s0)


def dpm_error(n, order=2):
    sch = DPMSolverMultistepSchedulerHIP(solver_order=order)
    sch.set_timesteps(n)
    rows = sch.coefficients()
    x_T = np.random.default_rng(0).standard_normal(4096)
    return float(np.abs(run_dpm(rows, x_T) - ode_target(x_T, float(rows[0, 0]), float(rows[0, 1]))).max())


def ddim_error(n):
    sch = DDIMSchedulerHIP()
    sch.set_timesteps(n)
    rows = np.asarray([sch.coefficients(int(t)) for t in sch.timesteps], dtype=np.float32)
    x_T = np.random.default_rng(0).standard_normal(4096)
    return float(np.abs(run_ddim(rows, x_T) - ode_target(x_T, float(rows[0, 0]), float(rows[0, 1]))).max())


def test_solver_accuracy_on_gaussian_data():
    e10, e15, e20 = dpm_error(10), dpm_error(15), dpm_error(20)
    ddim50 = ddim_error(50)
    print(f"max-abs error: DPM++2M 10/15/20 steps {e10:.3e} / {e15:.3e} / {e20:.3e}, DDIM-50 {ddim50:.3e}, "
          f"DDIM-20 {ddim_error(20):.3e}")
    assert e20 < 0.25 * ddim50
    assert e10 > e15 > e20
    for n in (20, 25):
        assert dpm_error(n, order=2) < dpm_error(n, order=1), n


# ---- config surface --------------------------------------------------------------------------------------------------
def test_config_round_trip(tmp_path):
    sch = DPMSolverMultistepSchedulerHIP(prediction_type="v_prediction", timestep_spacing="trailing", solver_order=1)
    sch.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "scheduler_config.json")) as f:
        d = json.load(f)
    assert d["_class_name"] == "DPMSolverMultistepScheduler"
    assert d["algorithm_type"] == "dpmsolver++" and d["solver_type"] == "midpoint" and d["solver_order"] == 1
    assert d["lower_order_final"] is True and d["euler_at_final"] is False and d["final_sigmas_type"] == "zero"
    assert d["use_karras_sigmas"] is False and d["thresholding"] is False and d["lambda_min_clipped"] == -math.inf
    back = DPMSolverMultistepSchedulerHIP.from_pretrained(str(tmp_path))
    assert vars(back.config) == vars(sch.config)
    for s in (sch, back):
        s.set_timesteps(12)
    assert np.array_equal(back.coefficients(), sch.coefficients())
    assert back.prediction_code == 1
    assert DPMSolverMultistepSchedulerHIP.from_config(DPMSolverMultistepSchedulerHIP.load_config(str(tmp_path))).solver_order == 1


def test_from_ddpm_config_inherits_spacing_and_offset():
    ddpm = DDPMSchedulerHIP(SchedulerConfig(steps_offset=1, prediction_type="sample"))
    sch = DPMSolverMultistepSchedulerHIP.from_config(ddpm.config)
    assert sch.config.timestep_spacing == "leading" and sch.config.steps_offset == 1
    assert sch.config.prediction_type == "sample" and sch.solver_order == 2
    sch.set_timesteps(20)
    assert np.array_equal(sch.timesteps.numpy(), ref_timesteps(20, "leading", offset=1))
    # add_noise is the base class's; DDPM / DDIM behave as before (their tables are their per-timestep coefficients)
    assert type(sch).add_noise is DDPMSchedulerHIP.add_noise
    ddim = DDIMSchedulerHIP()
    ddim.set_timesteps(50)
    want = np.asarray([ddim.coefficients(int(t)) for t in ddim.timesteps], dtype=np.float32)
    assert np.array_equal(ddim.sampler_table(), want)


@pytest.mark.parametrize("setting,value", [
    ("solver_order", 3), ("algorithm_type", "sde-dpmsolver++"), ("algorithm_type", "dpmsolver"), ("solver_type", "heun"),
    ("use_karras_sigmas", True), ("thresholding", True), ("timestep_spacing", "karras"), ("final_sigmas_type", "sigma_min"),
    ("lower_order_final", False), ("euler_at_final", True), ("lambda_min_clipped", -5.1),
])
def test_unsupported_settings_raise(setting, value):
    with pytest.raises(NotImplementedError, match=setting):
        DPMSolverMultistepSchedulerHIP(**{setting: value})


def test_step_count_without_distinct_timesteps_raises():
    sch = DPMSolverMultistepSchedulerHIP()
    with pytest.raises(ValueError):
        sch.set_timesteps(1000)                             # leading: 1000 // 1001 = 0, every timestep the same
    with pytest.raises(ValueError):
        sch.step(torch.zeros(1), 940, torch.zeros(1))       # (no timesteps set: the failed call left none)
