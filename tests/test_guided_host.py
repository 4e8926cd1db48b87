"""CPU: the host side of guided sampling on unconditional weights (RePaint-style known-region replacement) --
schedulers.repaint_program's row walk and coefficients, the latent mask, and what is refused."""
import numpy as np
import pytest
import torch

from rangeldm_amd.pipelines import latent_known_mask
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP, repaint_program

SCHEDULERS = (DDPMSchedulerHIP, DDIMSchedulerHIP)
PROGRAMS = ((50, 1, 1), (50, 10, 10), (20, 2, 2), (12, 3, 4), (7, 2, 3), (6, 6, 5), (5, 1, 3), (250, 10, 10))


def restated_walk(N, jl, jn):
    """RePaint's get_schedule_jump restated on time indices t = remaining - 1 (t = -1: the clean sample): the list of
    (remaining before the row, remaining after its re-noise)."""
    jumps = {j: jn - 1 for j in range(0, N - jl, jl)}
    t, rows = N, []
    while t >= 1:
        t -= 1                                       # denoise remaining t + 1 -> t
        start, end = t + 1, t
        if jumps.get(t - 1, 0) > 0:
            jumps[t - 1] -= 1
            end = t + jl
            t = end
        rows.append((start, end))
    return rows


@pytest.mark.parametrize("cls", SCHEDULERS)
@pytest.mark.parametrize("n", (1, 5, 50))
def test_no_resampling_is_the_schedulers_own_program(cls, n):
    sch = cls()
    ts, tab = repaint_program(sch, n)
    ref = cls()
    ref.set_timesteps(n)
    assert ts.dtype == torch.int64 and torch.equal(ts, ref.timesteps)
    assert tab.dtype == np.float32 and tab.shape == (n, 9) and tab.flags["C_CONTIGUOUS"]
    assert tab[:, :5].tobytes() == ref.sampler_table().tobytes()          # bit-equal, not close
    assert np.all(tab[:, 7] == 1.0) and np.all(tab[:, 8] == 0.0)
    # any jump_length without resampling is the same program
    ts2, tab2 = repaint_program(cls(), n, jump_length=3, jump_n_sample=1)
    assert torch.equal(ts2, ts) and tab2.tobytes() == tab.tobytes()


@pytest.mark.parametrize("N,jl,jn", PROGRAMS)
def test_row_count_and_walk(N, jl, jn):
    sch = DDPMSchedulerHIP()
    ts, tab = repaint_program(sch, N, jl, jn)
    points = len(range(0, N - jl, jl))
    assert len(ts) == N + (jn - 1) * jl * points == tab.shape[0]
    walk = restated_walk(N, jl, jn)
    assert len(walk) == len(ts)
    own = DDPMSchedulerHIP()
    own.set_timesteps(N)
    base = own.timesteps.tolist()
    assert ts.tolist() == [base[N - start] for start, _ in walk]
    jump_rows = [i for i, (start, end) in enumerate(walk) if end >= start]
    assert [i for i in range(len(ts)) if tab[i, 8] != 0.0] == jump_rows
    assert len(jump_rows) == (jn - 1) * points
    # every row's first five columns are the scheduler's own row of that timestep
    for i in (0, len(ts) // 2, len(ts) - 1):
        assert tab[i, :5].tobytes() == np.asarray(own.coefficients(int(ts[i])), dtype=np.float32).tobytes()


@pytest.mark.parametrize("cls", SCHEDULERS)
@pytest.mark.parametrize("N,jl,jn", PROGRAMS[1:5])
def test_blend_and_renoise_coefficients(cls, N, jl, jn):
    sch = cls()
    ts, tab = repaint_program(sch, N, jl, jn)
    ac = sch.alphas_cumprod.numpy().astype(np.float64)
    ratio = 1000 // N
    walk = restated_walk(N, jl, jn)
    t64 = tab.astype(np.float64)
    for i, (start, end) in enumerate(walk):
        t = int(ts[i])
        a_lo = ac[t - ratio] if t - ratio >= 0 else 1.0               # the level the scheduler's own step lands on
        np.testing.assert_allclose(t64[i, 5], np.sqrt(a_lo), rtol=2e-7, atol=0)
        np.testing.assert_allclose(t64[i, 6], np.sqrt(1 - a_lo), rtol=2e-7, atol=1e-9)
        assert abs(t64[i, 5] ** 2 + t64[i, 6] ** 2 - 1.0) < 4e-7
        if end < start:
            assert tab[i, 7] == 1.0 and tab[i, 8] == 0.0
            continue
        ra, rb = t64[i, 7], t64[i, 8]
        assert abs(ra * ra + rb * rb - 1.0) < 4e-7                    # fp32 rounding of two numbers <= 1
        own = cls()
        own.set_timesteps(N)
        a_hi = ac[int(own.timesteps[N - end])]
        assert a_hi < a_lo
        np.testing.assert_allclose(ra * ra * a_lo, a_hi, rtol=4e-7, atol=0)   # maps alpha_lo to alpha_hi
        if i + 1 < len(ts):
            assert int(ts[i + 1]) == int(own.timesteps[N - end])              # ... which is where the next row starts
    assert tab[-1, 5] == 1.0 and tab[-1, 6] == 0.0                            # the final sample is z0 on known pixels
    assert tab[-1, 7] == 1.0 and tab[-1, 8] == 0.0


def test_latent_mask_is_a_min_pool():
    g = torch.Generator().manual_seed(3)
    m = (torch.rand((2, 1, 32, 16), generator=g) > 0.08)
    m[0, :, 8:16, :] = True
    m[1, :, 4:8, 4:12] = True
    lat = latent_known_mask(m, 4)
    assert lat.shape == (2, 1, 8, 4) and lat.dtype == torch.float32
    want = m.float().reshape(2, 1, 8, 4, 4, 4).amin(dim=(3, 5))
    assert torch.equal(lat, want)
    assert 0 < lat.sum() < lat.numel()
    # an azimuth span: the pixels outside it are known, and so is every latent column that lies wholly outside
    span = torch.ones((1, 1, 1024, 64))
    span[:, :, 0:64] = 0
    lat = latent_known_mask(span, 4)
    assert lat.shape == (1, 1, 256, 16) and lat[0, 0, :16].sum() == 0 and bool((lat[0, 0, 16:] == 1).all())
    # float and bool masks agree
    assert torch.equal(latent_known_mask(span > 0.5, 4), lat)


def test_beam_subsampling_mask_raises_for_the_latent_pipeline():
    m = torch.zeros((2, 1, 1024, 64), dtype=torch.bool)
    m[..., 2::4] = True                                               # every 4th beam: densification
    with pytest.raises(ValueError, match="pixel-space"):
        latent_known_mask(m, 4)
    ok = torch.ones((2, 1, 1024, 64), dtype=torch.bool)
    ok[1] = m[1]                                                      # one sample of the batch is enough to refuse
    with pytest.raises(ValueError, match="DDIMPipelineRange"):
        latent_known_mask(ok, 4)
    with pytest.raises(ValueError):
        latent_known_mask(torch.ones((1, 1, 30, 16)), 4)


def test_dpmsolver_guided_is_refused():
    with pytest.raises(NotImplementedError, match="DPM-Solver"):
        repaint_program(DPMSolverMultistepSchedulerHIP(), 20)
    with pytest.raises(ValueError):
        repaint_program(DDPMSchedulerHIP(), 10, jump_length=0)
    with pytest.raises(ValueError):
        repaint_program(DDPMSchedulerHIP(), 10, jump_n_sample=0)


def test_binding_declares_the_guided_entry_points():
    from rangeldm_amd import _lib
    assert "rldm_sample_guided" in _lib.PROTOTYPES and "rldm_sched_guided_step" in _lib.PROTOTYPES
    # the newest field fills the alignment hole in front of `coef`: a zeroed struct is today's sampler, and no offset or size moved
    import ctypes
    assert _lib.SamplerConfigC.guided.offset == 20 and _lib.SamplerConfigC.coef.offset == 24
    assert ctypes.sizeof(_lib.SamplerConfigC) == 48
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rangeldm_hip.h")) as f:
        header = f.read()
    assert "int rldm_sample_guided(" in header and "int rldm_sched_guided_step(" in header
    body = header[header.index("typedef struct rldm_sampler_config"):header.index("} rldm_sampler_config;")]
    assert body.index("int32_t cond_channels;") < body.index("int32_t guided;") < body.index("const float* coef;")
