"""CPU: the fp64 reference of one scheduler step as conv_out's epilogue runs it (tests/test_sched_tail_exact.py holds the kernels to it,
bit for bit) -- checked against the oracle schedulers, and the exactness claim its bit-for-bit use rests on.

sched_tail_reference is written from the formulas of include/rangeldm_hip.h (rldm_sched_step / rldm_sched_dpmsolver_step), in float64:
  epsilon       x0 = (x - c1 * out) / c0        eps = out
  v_prediction  x0 = c0 * x - c1 * out          eps = c0 * out + c1 * x
  sample        x0 = out                        eps = (x - c0 * out) / c1
  DDIM          prev = c2 * x0 + c3 * eps + c4 * noise
  DDPM          prev = c2 * x0 + c3 * x   + c4 * noise
  DPM-Solver    prev = c2 * x0 + c3 * x   + c4 * x0_prev       (x0_prev: the history, which then receives x0)
The c4 term is absent when c4 == 0 (its operand is then not read: it may be NaN).

On the operand grids below every product, sum and quotient of every mode is exactly representable in fp32, so a kernel that fuses a
product into an fma and one that rounds it first agree, and the reference (rounded to fp32: no rounding) is the one right answer."""
import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd.config import SchedulerConfig

MODES = (_lib.RLDM_SAMPLER_DDIM, _lib.RLDM_SAMPLER_DDPM, _lib.RLDM_SAMPLER_DPMSOLVER)
MODE_NAMES = {_lib.RLDM_SAMPLER_DDIM: "ddim", _lib.RLDM_SAMPLER_DDPM: "ddpm", _lib.RLDM_SAMPLER_DPMSOLVER: "dpmsolver"}
PTYPES = ("epsilon", "v_prediction", "sample")          # RLDM_PRED_EPSILON / _V / _SAMPLE = the index

# ---- the exact-operand grids (group A of tests/test_sched_tail_exact.py) ---------------------------------------------------------------
EXACT_ROW = (0.5, 0.25, 1.5, -0.75, 0.5)                # c0 .. c4: powers of two and 3 * 2^-k, so no product gains more than 2 bits
EXACT_ROW_C4_ZERO = (0.5, 0.25, 1.5, -0.75, 0.0)
E_UNIT, E_MAX = 2.0 ** -8, 64.0                         # model output (the conv's fp32 result)
X_UNIT, X_MAX = 2.0 ** -3, 8.0                          # sample
Z_UNIT, Z_MAX = 2.0 ** -2, 4.0                          # noise / x0 history


def grid_draw(n, unit, vmax, seed):
    """n seeded multiples of `unit` in [-vmax, vmax] (float32), the two extremes among them."""
    g = torch.Generator().manual_seed(seed)
    k = int(round(vmax / unit))
    v = torch.randint(-k, k + 1, (n,), generator=g).to(torch.float64) * unit
    if n >= 2:
        v[0], v[-1] = vmax, -vmax
    return v.to(torch.float32)


def assert_grid(t, unit, vmax, what):
    q = np.asarray(t, dtype=np.float64) / unit
    assert np.array_equal(q, np.round(q)) and np.abs(q).max() * unit <= vmax, f"{what}: off the {unit} grid or above {vmax}"


def sched_tail_reference(mode, ptype, row, e, x, noise_or_hist, trace=None):
    """-> (x_prev, x0) in float64.  mode: RLDM_SAMPLER_*, ptype: RLDM_PRED_* (0 epsilon, 1 v_prediction, 2 sample), row: c0 .. c4.
    `trace` (a list) receives every intermediate product / sum / quotient, for the exactness assertion."""
    c0, c1, c2, c3, c4 = (float(v) for v in row)
    e, x = np.asarray(e, dtype=np.float64), np.asarray(x, dtype=np.float64)
    t = trace if trace is not None else []

    def k(v):
        t.append(v)
        return v

    if ptype == 0:
        x0 = k(k(x - k(c1 * e)) / c0)
        pe = e
    elif ptype == 1:
        x0 = k(k(c0 * x) - k(c1 * e))
        pe = k(k(c0 * e) + k(c1 * x))
    elif ptype == 2:
        x0 = e
        pe = k(k(x - k(c0 * e)) / c1)
    else:
        raise ValueError(ptype)
    second = pe if mode == _lib.RLDM_SAMPLER_DDIM else x
    prev = k(k(c2 * x0) + k(c3 * second))
    if c4 != 0.0:
        prev = k(prev + k(c4 * np.asarray(noise_or_hist, dtype=np.float64)))
    return prev, x0


def assert_trace_exact(trace, what):
    """every recorded intermediate equals its own fp32 rounding, and is finite"""
    worst = 0.0
    for i, v in enumerate(trace):
        assert np.isfinite(v).all(), f"{what}: intermediate {i} not finite"
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), f"{what}: intermediate {i} is not exact in fp32"
        worst = max(worst, float(np.abs(v).max()))
    return worst


# ---- the reference against the oracle schedulers ---------------------------------------------------------------------------------------
def _operands(seed, shape=(2, 3, 8, 4)):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(shape, generator=g) for _ in range(3))


@pytest.mark.parametrize("ptype", PTYPES)
def test_reference_matches_oracle_ddim_and_ddpm(ptype):
    from oracle.schedulers import OracleDDIMScheduler, OracleDDPMScheduler
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP
    cfg = SchedulerConfig(prediction_type=ptype)
    out, x, z = _operands(201)
    p = PTYPES.index(ptype)
    for t in (980, 500, 20):                                  # (t - 20 >= 0: both sides read alphas_cumprod for the previous step)
        d, do = DDIMSchedulerHIP(cfg), OracleDDIMScheduler(cfg)
        for eta in (0.0, 0.5):
            d.set_timesteps(50)
            do.set_timesteps(50)
            row = d.coefficients(t, eta)
            assert (row[4] != 0.0) == (eta != 0.0)
            want = do.step(out, t, x, eta=eta, noise=z)
            prev, x0 = sched_tail_reference(_lib.RLDM_SAMPLER_DDIM, p, row, out.numpy(), x.numpy(), z.numpy())
            assert np.abs(prev - want.prev_sample.double().numpy()).max() < 3e-5 * (1 + np.abs(prev).max()), (t, eta)
            assert np.abs(x0 - want.pred_original_sample.double().numpy()).max() < 3e-5 * (1 + np.abs(x0).max()), (t, eta)
    for t in (980, 500, 20, 0):
        s, so = DDPMSchedulerHIP(cfg), OracleDDPMScheduler(cfg)
        s.set_timesteps(50)
        so.set_timesteps(50)
        row = s.coefficients(t)
        assert (row[4] == 0.0) == (t == 0)
        want = so.step(out, t, x, noise=z)
        hole = np.full(tuple(z.shape), np.nan) if t == 0 else z.numpy()        # c4 == 0: the noise is not an operand
        prev, x0 = sched_tail_reference(_lib.RLDM_SAMPLER_DDPM, p, row, out.numpy(), x.numpy(), hole)
        assert np.isfinite(prev).all()
        assert np.abs(prev - want.prev_sample.double().numpy()).max() < 3e-5 * (1 + np.abs(prev).max()), t
        assert np.abs(x0 - want.pred_original_sample.double().numpy()).max() < 3e-5 * (1 + np.abs(x0).max()), t


@pytest.mark.parametrize("ptype", PTYPES)
def test_reference_matches_restated_dpmsolver(ptype):
    """the rows of DPMSolverMultistepSchedulerHIP.coefficients() through the reference, history carried as the kernels carry it, against
    RestatedDPM (float64, rows of its own derivation) stepping the same trajectory"""
    from rangeldm_amd.schedulers import DPMSolverMultistepSchedulerHIP
    from tests.test_dpmsolver_gpu import RestatedDPM
    n = 8
    sch = DPMSolverMultistepSchedulerHIP(SchedulerConfig(prediction_type=ptype))
    sch.set_timesteps(n)
    rows = sch.coefficients()
    assert rows.shape == (n, 5) and rows[0][4] == 0 and rows[3][4] != 0 and rows[n - 1][4] == 0
    ref = RestatedDPM(ptype)
    ref.set_timesteps(n)
    p = PTYPES.index(ptype)
    _, x, _ = _operands(202)
    xa, xb = x.numpy().astype(np.float64), x.clone()
    hist = np.full(xa.shape, np.nan)                           # (row 0 does not read it)
    for i in range(n):
        out = _operands(300 + i)[0]
        xa, hist = sched_tail_reference(_lib.RLDM_SAMPLER_DPMSOLVER, p, rows[i], out.numpy(), xa, hist)
        xb = ref.step(out, int(ref.timesteps[i]), xb).prev_sample
        assert np.isfinite(xa).all()
        assert np.abs(xa - xb.double().numpy()).max() < 3e-5 * (1 + np.abs(xa).max()), i


# ---- the exactness claim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", range(3), ids=PTYPES)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_every_intermediate_is_exact_on_the_operand_grids(mode, ptype):
    n = 200_000
    e, x, z = grid_draw(n, E_UNIT, E_MAX, 211), grid_draw(n, X_UNIT, X_MAX, 212), grid_draw(n, Z_UNIT, Z_MAX, 213)
    # the corners as well: every sign combination of the three extremes
    corners = np.array([[se * E_MAX, sx * X_MAX, sz * Z_MAX] for se in (-1, 1) for sx in (-1, 1) for sz in (-1, 1)], dtype=np.float32)
    e, x, z = (np.concatenate([t.numpy(), corners[:, i]]) for i, t in enumerate((e, x, z)))
    assert_grid(e, E_UNIT, E_MAX, "e")
    assert_grid(x, X_UNIT, X_MAX, "x")
    assert_grid(z, Z_UNIT, Z_MAX, "noise")
    for row in (EXACT_ROW, EXACT_ROW_C4_ZERO):
        assert all(float(np.float32(c)) == c for c in row)
        trace = []
        hole = np.full(z.shape, np.nan) if row[4] == 0.0 else z
        prev, x0 = sched_tail_reference(mode, ptype, row, e, x, hole, trace)
        worst = assert_trace_exact(trace + [prev, x0], f"{MODE_NAMES[mode]} {PTYPES[ptype]} row {row}")
        # the largest value any mode can reach: DDIM on a sample prediction, |eps| <= (8 + 0.5 * 64) / 0.25 = 160, so
        # |prev| <= 1.5 * 64 + 0.75 * 160 + 0.5 * 4 = 218 -- far inside fp32's 2^24 units of the finest grid in play (2^-12)
        assert worst <= 218.0 and 218.0 / 2.0 ** -12 < 2 ** 24
        assert len(trace) >= 3 + (2 if row[4] else 0)


def test_reference_distinguishes_the_modes():
    """the nine (mode, prediction) pairs give nine different x_prev on the exact operands -- a test that compares against this
    reference cannot pass with another pair's formula"""
    e, x, z = (grid_draw(64, u, m, s).numpy() for u, m, s in ((E_UNIT, E_MAX, 221), (X_UNIT, X_MAX, 222), (Z_UNIT, Z_MAX, 223)))
    outs = [sched_tail_reference(m, p, EXACT_ROW, e, x, z)[0] for m in MODES for p in range(3)]
    # DDPM and DPM-Solver share one formula (the third operand differs by where it comes from, not by the expression)
    for i, a in enumerate(outs):
        for j, b in enumerate(outs):
            same_formula = i == j or {i // 3, j // 3} == {1, 2} and i % 3 == j % 3
            assert np.array_equal(a, b) == same_formula, (i, j)
