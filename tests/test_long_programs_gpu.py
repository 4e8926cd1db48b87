"""GPU: the captured samplers (csrc/sampler.hip) on programs longer than anything else in the suite runs -- 67 rows (prime: one step
per graph, 67 replays), 130 (13 replays of 10), the 1000 rows of a pixel-space DDPM run (100 replays) and a guided program of 110
rows with jumps -- bit for bit against the same rows driven from the host.

Every step of a captured sampler finds its rows through the device step word: the coefficient row (5 floats, 9 when guided), the
row of every noise tensor (step * noise_step_stride), the Philox row of a sampler that draws in its graph, the time-embedding row,
the DPM-Solver++ history.  Elsewhere the suite stops at 50 rows and five replays.

The network here answers the same for every input: conv_out.weight = 0 and conv_out.bias on the 2^-3 grid, so eps == bias exactly
(asserted on a forward) whatever x and the time embedding are.  The final sample of a sampler is then a function of its rows alone,
and must equal the chain  x <- scheduler._launch(mode, table[k], eps, x, noise_k)  over the same sampler_table() rows (guided:
schedulers.guided_step; DPM-Solver++: rldm_sched_dpmsolver_step with its history tensor), the stand-alone launch that
tests/test_sched_tail_exact.py holds bit-equal to the fused tail and exact against fp64.  A row read at a wrong index, a noise or
Philox row off by any number of steps, a replay too many or too few changes the bits.  (The time-embedding rows do not reach the
result here; tests/test_temb_gpu.py has them.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib, rng
from rangeldm_amd.config import SchedulerConfig, UNetConfig
from rangeldm_amd.params import unet_param_shapes
from rangeldm_amd.schedulers import (DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP, guided_step,
                                     repaint_program)
from rangeldm_amd.synth import normal, synth_state_dict

pytestmark = pytest.mark.gpu
LAT = (4, 32, 8)
BIAS = (0.25, -0.5, 0.125, 0.375)               # conv_out.bias: multiples of 2^-3
SEED = (0xBADC0DE << 32) | 0x7654321
FLAGS = [0, int(_lib.Flag.SCHED_LAUNCH)]
FLAG_IDS = ["fused_tail", "sched_launch"]
_NET = {}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _unet():
    """the 32 x 8 network of the sampler tests (tests/test_hip_models.py's _small_unet) with an output layer that ignores its input"""
    from rangeldm_amd.unet import UNet2DModelHIP
    if "m" not in _NET:
        cfg = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64))
        sd = synth_state_dict(unet_param_shapes(cfg), prefix="long/small.")
        sd["conv_out.weight"] = np.zeros_like(sd["conv_out.weight"])
        sd["conv_out.bias"] = np.asarray(BIAS, dtype=np.float32)
        m = UNet2DModelHIP(cfg)
        m.load_state_dict(sd)
        _NET["m"] = m
    return _NET["m"]


def _eps(B):
    return torch.tensor(BIAS).view(1, 4, 1, 1).expand(B, *LAT).contiguous().cuda()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_same(got, want, what):
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), f"{what}: not finite"
    n = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert n == 0, (f"{what}: {n} of {got.numel()} elements of the captured sampler's result differ in bits from the host-driven chain over "
                    f"the same rows (max |diff| {float((got - want).abs().max()):.3g})")


def _sampler(fs, sch, B, steps, mode, flags, program=None):
    return fs.get(_unet(), None, sch, B, steps, mode, True, 0, program=program, plan_flags=flags)


def _chain(sch, mode, table, x_T, eps, noise):
    """noise: k -> the row's noise tensor (asked only where table[k][4] != 0)"""
    x = x_T.clone()
    for k in range(len(table)):
        x = sch._launch(mode, table[k], eps, x, noise(k) if float(table[k][4]) != 0.0 else None)
    return x


def _host_rows(shape, draw, purpose, rows, offset):
    """[rows, *shape] on the device: row r = rng.randn_host at (SEED, draw, purpose, r), the generator's host statement"""
    return T(np.stack([rng.randn_host(shape, SEED, draw, purpose, r, offset) for r in range(rows)])).cuda()


def test_network_output_is_its_bias_exactly():
    m = _unet()
    x = T(normal(3, "long/x", (2, 5, 32, 8))).cuda()
    for t in (999, 0):
        assert torch.equal(m(x, t).sample, _eps(2)), t
    assert torch.equal(m(x * 7 - 3, torch.tensor([5, 700])).sample, _eps(2))
    assert float(torch.tensor(BIAS).mul(8).frac().abs().max()) == 0.0


# ---- DDPM: injected noise and the generator's, fused tail and separate launches, one chain and two lanes --------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("steps,B,lanes", [(67, 2, 1), (67, 4, 2), (130, 2, 1), (1000, 2, 1)],
                         ids=["67", "67-two_lanes", "130", "1000"])
def test_ddpm_sampler_equals_the_host_chain(steps, B, lanes, flags, monkeypatch):
    from rangeldm_amd.pipelines import _FusedSampler
    monkeypatch.setenv("RLDM_LANES", str(lanes))
    sch = DDPMSchedulerHIP()
    fs = _FusedSampler()
    h = _sampler(fs, sch, B, steps, _lib.RLDM_SAMPLER_DDPM, flags)
    table = sch.sampler_table()
    assert table.shape == (steps, 5) and (table[:-1, 4] != 0).all() and table[-1, 4] == 0 and len(np.unique(table[:, 0])) == steps
    shape, eps = (B, *LAT), _eps(B)
    what = f"DDPM {steps} steps, B = {B}, {lanes} lane(s), {'separate launches' if flags else 'fused tail'}"
    # injected step_noise
    x_T = T(normal(11, f"long/xT/{steps}", shape)).cuda()
    zs = T(normal(11, f"long/zs/{steps}", (steps, *shape))).cuda()
    lat = torch.empty(shape, device="cuda")
    fs.run(h, x_T, zs, None, None, latents_out=lat)
    assert fs.captures(h) >= lanes
    want = _chain(sch, 1, table, x_T, eps, lambda k: zs[k])
    _assert_same(lat, want, what + ", injected noise")
    assert not _same(lat, _chain(sch, 1, table, x_T, eps, lambda k: zs[(k + 64) % steps]))        # (the rows do differ)
    # the sampler draws x_T and every row itself: (SEED, draw 3), samples offset + b
    draw, offset = 3, 9
    lat_r = torch.empty(shape, device="cuda")
    fs.run_rng(h, None, SEED, draw, offset, None, None, latents_out=lat_r)
    x_T = T(rng.randn_host(shape, SEED, draw, 0, 0, offset)).cuda()
    zr = _host_rows(shape, draw, 1, steps, offset)
    _assert_same(lat_r, _chain(sch, 1, table, x_T, eps, lambda k: zr[k]), what + ", rng.DeviceGenerator")
    assert not _same(lat_r, lat)


# ---- DDIM (each prediction type) and DPM-Solver++ (the history) -----------------------------------------------------------
@pytest.mark.parametrize("steps,ptype", [(67, "epsilon"), (130, "v_prediction"), (67, "sample"), (130, "sample")])
def test_ddim_sampler_equals_the_host_chain(steps, ptype):
    from rangeldm_amd.pipelines import _FusedSampler
    sch = DDIMSchedulerHIP(SchedulerConfig(prediction_type=ptype))
    fs = _FusedSampler()
    B = 2
    h = _sampler(fs, sch, B, steps, _lib.RLDM_SAMPLER_DDIM, 0)
    table = sch.sampler_table(0.0)
    assert table.shape == (steps, 5) and (table[:, 4] == 0).all() and len(np.unique(table[:, 0])) == steps
    x_T = T(normal(12, f"long/ddim/{steps}", (B, *LAT))).cuda()
    lat = torch.empty_like(x_T)
    fs.run(h, x_T, None, None, None, latents_out=lat)
    _assert_same(lat, _chain(sch, 0, table, x_T, _eps(B), None), f"DDIM {steps} steps, {ptype}")


def _dpm_chain(sch, table, x_T, eps):
    x, hist = x_T.clone(), torch.zeros_like(x_T)
    for row in table:
        out = torch.empty_like(x)
        cf = (C.c_float * 5)(*[float(v) for v in row])
        _lib.check(_lib.lib().rldm_sched_dpmsolver_step(sch.prediction_code, cf, C.c_void_p(eps.data_ptr()), C.c_void_p(x.data_ptr()),
                                                        C.c_void_p(hist.data_ptr()), C.c_void_p(out.data_ptr()), x.numel(),
                                                        _lib.stream_ptr(x.device)), "DPM-Solver++ step")
        x = out
    return x


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("steps", [67, 130])
def test_dpmsolver_sampler_equals_the_host_chain(steps, flags):
    from rangeldm_amd.pipelines import _FusedSampler
    sch = DPMSolverMultistepSchedulerHIP()
    fs = _FusedSampler()
    B = 2
    h = _sampler(fs, sch, B, steps, _lib.RLDM_SAMPLER_DPMSOLVER, flags)
    table = sch.sampler_table()
    assert table.shape == (steps, 5) and table[0, 4] == 0 and (table[1:-1, 4] != 0).all()        # every inner row reads the history
    x_T = T(normal(13, f"long/dpm/{steps}", (B, *LAT))).cuda()
    lat = torch.empty_like(x_T)
    fs.run(h, x_T, None, None, None, latents_out=lat)
    _assert_same(lat, _dpm_chain(sch, table, x_T, _eps(B)), f"DPM-Solver++ {steps} steps, {'separate launches' if flags else 'fused tail'}")


# ---- a guided program with jumps -------------------------------------------------------------------------------------------
def test_guided_ddpm_program_with_jumps_equals_the_host_chain():
    """40 steps, jump_length 5, jump_n_sample 3: 7 jump points, 40 + 2 * 5 * 7 = 110 rows of 9, re-noise on 14 of them; the noise of
    all three purposes once as tensors and once drawn in the graph."""
    from rangeldm_amd.pipelines import _FusedSampler
    sch = DDPMSchedulerHIP()
    ts, table = repaint_program(sch, 40, 5, 3)
    rows = len(ts)
    assert rows == 110 and table.shape == (110, 9)
    jumps = (table[:, 7] != 1.0) | (table[:, 8] != 0.0)
    assert int(jumps.sum()) == 14 and jumps[64:].any() and (table[64:, 6] != 0).any() and (table[64:, 4] != 0).any()
    B = 2
    shape, eps = (B, *LAT), _eps(B)
    fs = _FusedSampler()
    h = _sampler(fs, sch, B, rows, _lib.RLDM_SAMPLER_DDPM, 0, program=(ts, table))
    z0 = T(normal(14, "long/z0", shape)).cuda()
    mask = torch.ones((B, 1, 32, 8), device="cuda")
    mask[:, :, 5:21] = 0
    mask[1, :, :, 3] = 0

    def chain(x_T, zs, nk, nr):
        x = x_T.clone()
        for k in range(rows):
            x = guided_step(sch, table[k], eps, x, zs[k], z0, mask, nk[k], nr[k])
        return x
    sel = mask.expand(shape) == 1
    # the three noise tensors given
    x_T = T(normal(14, "long/xT", shape)).cuda()
    zs, nk, nr = (T(normal(14, f"long/guided/{k}", (rows, *shape))).cuda() for k in ("zs", "nk", "nr"))
    lat = torch.empty(shape, device="cuda")
    fs.run_guided(h, x_T, zs, z0, mask, nk, nr, None, latents_out=lat)
    _assert_same(lat, chain(x_T, zs, nk, nr), "guided DDPM, 110 rows, noise tensors given")
    assert _same(lat[sel], z0[sel]) and not _same(lat[~sel], z0[~sel])
    # drawn in the graph
    draw, offset = 2, 4
    lat_r = torch.empty(shape, device="cuda")
    fs.run_guided_rng(h, None, SEED, draw, offset, z0, mask, None, latents_out=lat_r)
    x_T = T(rng.randn_host(shape, SEED, draw, 0, 0, offset)).cuda()
    zs, nk, nr = (_host_rows(shape, draw, q, rows, offset) for q in (1, 2, 3))
    _assert_same(lat_r, chain(x_T, zs, nk, nr), "guided DDPM, 110 rows, rng.DeviceGenerator")
    assert _same(lat_r[sel], z0[sel]) and not _same(lat_r, lat)
