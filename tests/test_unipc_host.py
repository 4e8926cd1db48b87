"""CPU: UniPCMultistepSchedulerHIP's host side -- the coefficient rows against a float64 restatement of diffusers'
UniPCMultistepScheduler (bh2, predict_x0, lower_order_final, final_sigmas_type "zero") written as diffusers writes it (lists of model
outputs, one predictor and one corrector update), the anchor to DPM-Solver++(2M), the solver's order of accuracy on the Gaussian
problem of tests/test_dpmsolver_host.py, and the config surface."""
import json
import math
import os

import numpy as np
import pytest
import torch

from rangeldm_amd.config import SchedulerConfig
from rangeldm_amd.schedulers import DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP, UniPCMultistepSchedulerHIP
from tests.test_dpmsolver_host import MU, SD, SPACINGS, alphas_cumprod, dpm_error, exact_eps, ode_target, ref_timesteps

STEP_COUNTS = (1, 2, 3, 4, 10, 25)
ORDERS = (1, 2, 3)
ROW = ("alpha", "s", "use_corr", "k_last", "k_1", "k_2", "k_3", "k_t", "p_x", "p_0", "p_1", "p_2")


# ---- the restatement (float64 from the fp32 alphas_cumprod) -------------------------------------------------------------
def ref_grid(ts):
    """alpha, s, lambda at the n timesteps and behind the last one (s = 0, alpha = 1, lambda = +inf)"""
    ac = alphas_cumprod()[np.asarray(ts)]
    sig = np.append(np.sqrt((1 - ac) / ac), 0.0)
    alpha = 1 / np.sqrt(sig ** 2 + 1)
    s = sig * alpha
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(s)
    return alpha, s, lam


def uni_update(grid, j, t, x, m0, older, order, m_t=None):
    """One UniP (m_t None) or UniC (m_t: the x0 prediction at t) update of order `order` from grid index j to t.  m0: the x0 prediction
    at j; older[k - 1]: the one at j - k.  x, m0, older, m_t: anything numpy or torch can add and scale."""
    alpha, s, lam = grid
    if s[t] == 0.0:
        return m0                                            # into sigma = 0: phi1 = -1, first order
    h = lam[t] - lam[j]
    hh = -h
    phi1 = math.expm1(hh)
    B = math.expm1(hh)                                       # B(h) = e^h - 1 ("bh2") in data-prediction form
    rks = [(lam[j - k] - lam[j]) / h for k in range(1, order)]
    D1s = [(older[k - 1] - m0) / rks[k - 1] for k in range(1, order)]
    rks.append(1.0)
    R, b = [], []
    hphi, fact = phi1 / hh - 1, 1
    for jj in range(1, order + 1):
        R.append([r ** (jj - 1) for r in rks])
        b.append(hphi * fact / B)
        fact *= jj + 1
        hphi = hphi / hh - 1 / fact
    R, b = np.asarray(R, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if m_t is None:
        rho = [] if order == 1 else [0.5] if order == 2 else list(np.linalg.solve(R[:-1, :-1], b[:-1]))
    else:
        rho = [0.5] if order == 1 else list(np.linalg.solve(R, b))
    out = (s[t] / s[j]) * x - (alpha[t] * phi1) * m0
    for k in range(order - 1):
        out = out - (alpha[t] * B * rho[k]) * D1s[k]
    if m_t is not None:
        out = out - (alpha[t] * B * rho[-1]) * (m_t - m0)
    return out


def ref_orders(n, solver_order):
    return [min(solver_order, n - i, i + 1) for i in range(n)]


class RestatedUniPC:
    """UniPC on the host in float64, as diffusers' scheduler keeps its state: for this file's tests and the oracle loops of
    tests/test_unipc_gpu.py."""
    init_noise_sigma = 1.0

    def __init__(self, prediction_type="epsilon", order=2, spacing="leading", disable_corrector=(), offset=0):
        self.ptype, self.order, self.spacing, self.offset = prediction_type, order, spacing, offset
        self.disabled = set(disable_corrector)

    def set_timesteps(self, n, device=None):
        ts = ref_timesteps(n, self.spacing, self.offset)
        self.grid = ref_grid(ts)
        self.timesteps = torch.from_numpy(np.ascontiguousarray(ts))
        self.n, self.i, self.taken = n, 0, 0
        self.m, self.last, self.prev_order = [], None, None

    def scale_model_input(self, x, t=None):
        return x

    def convert(self, out, x):
        a, s = self.grid[0][self.i], self.grid[1][self.i]
        return {"epsilon": lambda: (x - s * out) / a, "v_prediction": lambda: a * x - s * out, "sample": lambda: out}[self.ptype]()

    def advance(self, out, x):
        """-> (x_c, x_next): the corrected sample at this step and the predicted one at the next"""
        i = self.i
        m = self.convert(out, x)                             # (with the sample the network saw: the uncorrected one)
        x_c = x
        if self.taken >= 1 and (i - 1) not in self.disabled:
            x_c = uni_update(self.grid, i - 1, i, self.last, self.m[0], self.m[1:], self.prev_order, m_t=m)
        order = min(self.order, self.n - i, self.taken + 1)
        x_next = uni_update(self.grid, i, i + 1, x_c, m, self.m, order)
        self.m, self.last, self.prev_order = [m] + self.m[:2], x_c, order
        self.i, self.taken = i + 1, self.taken + 1
        return x_c, x_next

    def step(self, out, t, x, generator=None, noise=None):
        from types import SimpleNamespace
        return SimpleNamespace(prev_sample=self.advance(out.double(), x.double())[1].float())


def ref_rows(n, spacing, order, disabled=(), offset=0):
    """The [n][12] rows, read off the restated updates by running them on basis vectors (every term is linear in the tensors)."""
    grid = ref_grid(ref_timesteps(n, spacing, offset))
    orders = ref_orders(n, order)
    rows = np.zeros((n, 12))
    eye = np.eye(5)
    for i in range(n):
        rows[i, 0], rows[i, 1] = grid[0][i], grid[1][i]
        if i >= 1 and (i - 1) not in disabled:
            last, m1, m2, m3, mt = eye                       # x_c over (last, m_{i-1}, m_{i-2}, m_{i-3}, m_i)
            rows[i, 2] = 1.0
            rows[i, 3:8] = uni_update(grid, i - 1, i, last, m1, [m2, m3], orders[i - 1], m_t=mt)
        xc, mt, m1, m2, _ = eye                              # x_next over (x_c, m_i, m_{i-1}, m_{i-2})
        rows[i, 8:12] = uni_update(grid, i, i + 1, xc, mt, [m1, m2], orders[i])[:4]
    return rows, orders


def make(n, **kw):
    sch = UniPCMultistepSchedulerHIP(**kw)
    sch.set_timesteps(n)
    return sch


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", STEP_COUNTS)
def test_rows_match_restatement(n, spacing, order):
    sch = make(n, timestep_spacing=spacing, solver_order=order)
    assert np.array_equal(sch.timesteps.numpy(), ref_timesteps(n, spacing)) and sch.timesteps.dtype == torch.int64
    tab = sch.coefficients()
    assert tab.dtype == np.float32 and tab.shape == (n, 12) and tab.flags["C_CONTIGUOUS"]
    assert sch.sampler_table() is tab
    rows, orders = ref_rows(n, spacing, order)
    np.testing.assert_allclose(tab.astype(np.float64), rows, rtol=1e-6, atol=1e-10)
    if n >= 10:
        assert orders[:3] == [1, min(order, 2), order] and orders[3:-2] == [order] * (n - 5)     # warm-up 1, 2, 3
    assert orders[-1] == 1 and (n < 2 or orders[-2] == min(order, 2, n - 1))   # ..., 2, 1 at the end (the warm-up caps a short run)
    # what a step does not use is exactly 0: the corrector at step 0, history slots beyond the step's order
    assert list(tab[0, 2:8]) == [0.0] * 6
    assert list(tab[-1, 8:]) == [0.0, 1.0, 0.0, 0.0]                           # the last step returns m
    for i in range(n):
        assert tab[i, 2] == (1.0 if i >= 1 else 0.0)
        assert [tab[i, 10] != 0, tab[i, 11] != 0] == [orders[i] >= 2, orders[i] >= 3], i
        if i >= 1:
            assert [tab[i, 5] != 0, tab[i, 6] != 0] == [orders[i - 1] >= 2, orders[i - 1] >= 3], i
            assert tab[i, 3] != 0 and tab[i, 4] != 0 and tab[i, 7] != 0


@pytest.mark.parametrize("disabled", [[0], [1, 2], [0, 3, 8], list(range(10))])
def test_disabled_corrector_rows(disabled):
    sch = make(10, solver_order=3, disable_corrector=disabled)
    tab = sch.coefficients()
    rows, _ = ref_rows(10, "leading", 3, disabled)
    np.testing.assert_allclose(tab.astype(np.float64), rows, rtol=1e-6, atol=1e-10)
    for i in range(10):
        off = i == 0 or (i - 1) in disabled
        assert tab[i, 2] == (0.0 if off else 1.0)
        if off:
            assert list(tab[i, 3:8]) == [0.0] * 5
    # the predictor does not depend on the corrector
    assert np.array_equal(tab[:, 8:], make(10, solver_order=3).coefficients()[:, 8:])


def test_steps_offset_and_restated_stepper_agree_with_rows():
    """The rows applied as the kernel applies them reproduce the restated scheduler (state kept the way diffusers keeps it) on
    random tensors, through every order transition, for every prediction type."""
    rng = np.random.default_rng(3)
    for ptype in ("epsilon", "v_prediction", "sample"):
        sch = make(7, solver_order=3, steps_offset=1, prediction_type=ptype, disable_corrector=[2])
        ref = RestatedUniPC(ptype, 3, "leading", [2], offset=1)
        ref.set_timesteps(7)
        assert np.array_equal(sch.timesteps.numpy(), ref.timesteps.numpy())
        x = rng.standard_normal(64)
        xr = x.copy()
        last, hist = np.full(64, np.nan), [np.full(64, np.nan)] * 3
        for row in sch.coefficients().astype(np.float64):
            out = rng.standard_normal(64)
            x_c, x, m = apply_row(row, ptype, out, x, last, hist)
            last, hist = x_c, [m, hist[0], hist[1]]
            xc_ref, xr = ref.advance(out, xr)
            assert np.isfinite(x).all()
            np.testing.assert_allclose(x_c, xc_ref, rtol=0, atol=2e-6 * (1 + np.abs(xc_ref).max()))
            np.testing.assert_allclose(x, xr, rtol=0, atol=2e-6 * (1 + np.abs(xr).max()))
            xr = x.copy()                                   # (teacher-forced: fp32 rows against fp64 ones, one step at a time)
            ref.last = x_c


def apply_row(row, ptype, out, x, last, hist):
    """One row as sched_unipc_kernel applies it, in float64: -> (x_c, x_next, m).  A coefficient of 0 reads nothing."""
    a, s, use_corr, k_last, k_1, k_2, k_3, k_t, p_x, p_0, p_1, p_2 = row
    m = {"epsilon": lambda: (x - s * out) / a, "v_prediction": lambda: a * x - s * out, "sample": lambda: out}[ptype]()
    x_c = x
    if use_corr != 0:
        x_c = k_last * last + k_t * m
        for k, h in zip((k_1, k_2, k_3), hist):
            if k != 0:
                x_c = x_c + k * h
    x_next = p_x * x_c + p_0 * m
    for p, h in zip((p_1, p_2), hist):
        if p != 0:
            x_next = x_next + p * h
    return x_c, x_next, m


# ---- the anchor: UniP-2 is DPM-Solver++(2M), UniP-1 its first-order step --------------------------------------------------
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", (2, 3, 10, 25))
@pytest.mark.parametrize("order", (1, 2))
def test_predictor_only_is_dpmsolver(n, spacing, order):
    uni = make(n, timestep_spacing=spacing, solver_order=order, disable_corrector=list(range(n)))
    dpm = DPMSolverMultistepSchedulerHIP(timestep_spacing=spacing, solver_order=order)
    dpm.set_timesteps(n)
    ts = dpm.timesteps.numpy()
    r64 = uni._rows(ts)                                      # float64, before the fp32 rounding
    d64 = dpm._rows(ts, order)
    assert np.all(r64[:, 2:8] == 0.0) and np.all(r64[:, 11] == 0.0)
    np.testing.assert_allclose(r64[:, (0, 1)], d64[:, (0, 1)], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r64[:, (9, 8, 10)], d64[:, (2, 3, 4)], rtol=1e-12, atol=0)
    assert np.array_equal(uni.coefficients()[:, (0, 1, 9, 8, 10)], dpm.coefficients())      # hence the same fp32 rows


# ---- accuracy: Gaussian data, exact epsilon, exact probability-flow ODE solution ------------------------------------------
def run_unipc(rows, x, stop=None):
    last, hist = None, [None] * 3
    for row in rows.astype(np.float64)[:stop]:
        out = exact_eps(x, row[0], row[1])
        x_c, x, m = apply_row(row, "epsilon", out, x, last, hist)
        last, hist = x_c, [m, hist[0], hist[1]]
    return x


def ode_state(x_T, a0, s0, a, s):
    """The exact solution at (a, s) of the probability-flow ODE that starts from x_T at (a0, s0); (1, 0) gives ode_target"""
    z = (ode_target(x_T, a0, s0) - MU) / SD
    return a * MU + math.sqrt(a * a * SD * SD + s * s) * z


def unipc_error(n, order, corrector=True, at=None):
    """max-abs error of the fp32 rows run in float64 after `at` steps (None: all n, into sigma = 0)"""
    sch = make(n, solver_order=order, disable_corrector=[] if corrector else list(range(n)))
    rows = sch.coefficients()
    x_T = np.random.default_rng(0).standard_normal(4096)
    a0, s0 = float(rows[0, 0]), float(rows[0, 1])
    got = run_unipc(rows, x_T, at)
    if at is None or at == n:
        return float(np.abs(got - ode_target(x_T, a0, s0)).max())
    return float(np.abs(got - ode_state(x_T, a0, s0, float(rows[at, 0]), float(rows[at, 1]))).max())


def test_ode_state_ends_at_ode_target():
    x = np.linspace(-3, 3, 7)
    np.testing.assert_allclose(ode_state(x, 0.1, math.sqrt(0.99), 1.0, 0.0), ode_target(x, 0.1, math.sqrt(0.99)), rtol=1e-14)
    np.testing.assert_allclose(ode_state(x, 0.1, math.sqrt(0.99), 0.1, math.sqrt(0.99)), x, rtol=1e-14)


def test_order_of_accuracy_on_gaussian_data():
    """The error after the first 3n/4 steps (the last step, into sigma = 0, is first order for every solver and would set the
    ratio): halving the step divides it by 2^p."""
    def ratio(order, corrector):
        e40, e80 = (unipc_error(n, order, corrector, at=3 * n // 4) for n in (40, 80))
        print(f"order {order} corrector {corrector}: e(40) {e40:.3e} e(80) {e80:.3e} ratio {e40 / e80:.2f}")
        return e40 / e80
    assert ratio(1, False) >= 2 ** 0.5
    assert ratio(2, False) >= 2 ** 1.5
    assert ratio(2, True) >= 2 ** 2.5


def dpm_error_at(n, at):
    """DPMSolverMultistepSchedulerHIP's own rows on the same problem, after `at` steps (dpm_error(n) is the figure after all n)"""
    dpm = DPMSolverMultistepSchedulerHIP()
    dpm.set_timesteps(n)
    rows = dpm.coefficients()
    x_T = np.random.default_rng(0).standard_normal(4096)
    x, x0_prev = x_T, np.zeros_like(x_T)
    for a, s, c_x0, c_xt, c_x0p in rows.astype(np.float64)[:at]:
        x0 = (x - s * exact_eps(x, a, s)) / a
        x, x0_prev = c_x0 * x0 + c_xt * x + c_x0p * x0_prev, x0
    return float(np.abs(x - ode_state(x_T, float(rows[0, 0]), float(rows[0, 1]), float(rows[at, 0]), float(rows[at, 1]))).max())


@pytest.mark.parametrize("n", (10, 20, 40))
def test_unipc_beats_dpmsolver_and_order3_beats_order2(n):
    """Measured after the first 3n/4 steps, like the order.  Into sigma = 0 the comparison says nothing about the solvers: the leading
    grid ends with steps of h = 0.28, 0.38, 0.61 and infinity at every n, the last of them first order for all, and the errors there
    are 2M / UniPC-2 / UniPC-3 = 2.1e-1 / 1.7e-1 / 1.5e-1 (n = 10), 1.5e-2 / 1.6e-2 / 2.5e-2 (20), 9.4e-3 / 4.4e-4 / 1.1e-2 (40):
    printed below, not asserted (nor is the 3n/4 figure held against dpm_error(n), which is 2M after all n steps)."""
    at = 3 * n // 4
    e2m, u2, u3 = dpm_error_at(n, at), unipc_error(n, 2, at=at), unipc_error(n, 3, at=at)
    print(f"{n} steps, max-abs error after {at}: DPM++2M {e2m:.3e}  UniPC-2 {u2:.3e}  UniPC-3 {u3:.3e};  into sigma = 0: "
          f"DPM++2M {dpm_error(n):.3e}  UniPC-2 {unipc_error(n, 2):.3e}  UniPC-3 {unipc_error(n, 3):.3e}")
    assert u2 < e2m                                           # like for like: both after `at` steps (dpm_error(n) is only printed)
    assert u3 < u2
    # UniP-2 alone IS 2M, at the intermediate index and at the end
    assert abs(unipc_error(n, 2, corrector=False, at=at) - e2m) <= 1e-12 * (1 + e2m)
    assert abs(unipc_error(n, 2, corrector=False) - dpm_error(n)) <= 1e-12 * (1 + dpm_error(n))


# ---- the public step, on the CPU side of it: indices, state, refusals ------------------------------------------------------
def test_set_timesteps_resets_and_step_needs_timesteps():
    sch = UniPCMultistepSchedulerHIP()
    with pytest.raises(ValueError):
        sch.step(torch.zeros(1), 940, torch.zeros(1))
    sch.set_timesteps(10)
    assert sch.step_index is None and sch.init_noise_sigma == 1.0
    x = torch.randn(2, 3)
    assert sch.scale_model_input(x, 940) is x
    with pytest.raises(ValueError, match="not in scheduler.timesteps"):
        sch.step(torch.zeros(1), 941, torch.zeros(1))
    with pytest.raises(ValueError):
        sch.set_timesteps(1000)


# ---- config surface --------------------------------------------------------------------------------------------------
def test_config_round_trip(tmp_path):
    sch = UniPCMultistepSchedulerHIP(prediction_type="v_prediction", timestep_spacing="trailing", solver_order=3, disable_corrector=[0, 4])
    sch.save_pretrained(str(tmp_path))
    with open(os.path.join(str(tmp_path), "scheduler_config.json")) as f:
        d = json.load(f)
    assert d["_class_name"] == "UniPCMultistepScheduler"
    assert d["solver_type"] == "bh2" and d["solver_order"] == 3 and d["predict_x0"] is True and d["disable_corrector"] == [0, 4]
    assert d["lower_order_final"] is True and d["final_sigmas_type"] == "zero" and d["solver_p"] is None
    assert d["use_karras_sigmas"] is False and d["thresholding"] is False
    back = UniPCMultistepSchedulerHIP.from_pretrained(str(tmp_path))
    assert vars(back.config) == vars(sch.config)
    for s in (sch, back):
        s.set_timesteps(12)
    assert np.array_equal(back.coefficients(), sch.coefficients())
    assert back.prediction_code == 1
    assert UniPCMultistepSchedulerHIP.from_config(UniPCMultistepSchedulerHIP.load_config(str(tmp_path))).solver_order == 3


def test_from_ddpm_config_inherits_spacing_and_offset():
    ddpm = DDPMSchedulerHIP(SchedulerConfig(steps_offset=1, prediction_type="sample"))
    sch = UniPCMultistepSchedulerHIP.from_config(ddpm.config)
    assert sch.config.timestep_spacing == "leading" and sch.config.steps_offset == 1
    assert sch.config.prediction_type == "sample" and sch.solver_order == 2 and sch.config.disable_corrector == []
    sch.set_timesteps(20)
    assert np.array_equal(sch.timesteps.numpy(), ref_timesteps(20, "leading", offset=1))
    assert type(sch).add_noise is DDPMSchedulerHIP.add_noise
    # ... and from a DPM-Solver++ config: its own solver settings (solver_type "midpoint", algorithm_type) are not UniPC's
    dpm = DPMSolverMultistepSchedulerHIP(timestep_spacing="trailing", solver_order=1)
    sch = UniPCMultistepSchedulerHIP.from_config(dpm.config, solver_order=3)
    assert sch.config.timestep_spacing == "trailing" and sch.solver_order == 3 and sch.config.solver_type == "bh2"


@pytest.mark.parametrize("setting,value", [
    ("solver_order", 4), ("solver_order", 0), ("solver_type", "bh1"), ("predict_x0", False), ("thresholding", True),
    ("use_karras_sigmas", True), ("lower_order_final", False), ("final_sigmas_type", "sigma_min"), ("solver_p", object()),
    ("beta_schedule", "scaled_linear"), ("timestep_spacing", "karras"),
])
def test_unsupported_settings_raise(setting, value):
    with pytest.raises(NotImplementedError, match=setting):
        UniPCMultistepSchedulerHIP(**{setting: value})


def test_sampler_mode_and_guided_refusals():
    from rangeldm_amd import _lib
    from rangeldm_amd.guidance import refuse_unsupported
    from rangeldm_amd.schedulers import guided_step, repaint_program, sampler_mode
    sch = UniPCMultistepSchedulerHIP()
    assert _lib.RLDM_SAMPLER_UNIPC == 3 and sampler_mode(sch) == _lib.RLDM_SAMPLER_UNIPC
    assert sampler_mode(DPMSolverMultistepSchedulerHIP()) == _lib.RLDM_SAMPLER_DPMSOLVER
    with pytest.raises(NotImplementedError, match="history"):
        repaint_program(sch, 10)
    with pytest.raises(NotImplementedError, match="DDPM or DDIM"):
        guided_step(sch, np.zeros(9, dtype=np.float32), None, None, None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="DDIMSchedulerHIP"):
        refuse_unsupported(sch, 0.0, 1, 1, True)
