"""GPU: the counter-based generator (csrc/rng.hip) against its numpy statement (rangeldm_amd/rng.py), bit for bit -- the Philox block,
the written-out transform on chosen bits, rng.randn -- and everything built on it against its explicit twin: the captured samplers
that draw inside their step graph (rldm_sample_rng / rldm_sample_guided_rng) against the existing entry points fed with rng.randn
tensors, the pipelines, the trainers and the sampling drivers.  The twins run the same kernels on the same inputs: no tolerance."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib, rng
from rangeldm_amd.config import UNetConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.schedulers import (DDIMSchedulerHIP, DDPMSchedulerHIP, DPMSolverMultistepSchedulerHIP, randn_tensor,
                                     repaint_program)
from rangeldm_amd.synth import normal, synth_state_dict
from tests.hip_util import hip_unet, hip_vae, small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0xC0FFEE << 32) | 0x1234567        # >= 2^32: both key words are live
LAT = (4, 32, 8)                            # a latent of the small UNet below


def T(a):
    return torch.from_numpy(np.asarray(a))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- the block and the transform ------------------------------------------------------------------------------------------
def dev_philox(counters, key):
    c = T(np.ascontiguousarray(counters, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.empty_like(c)
    k = (C.c_uint32 * 2)(int(key[0]), int(key[1]))
    _lib.check(_lib.lib().rldm_rng_philox(p(c), k, c.shape[0], p(out), _lib.stream_ptr(c.device)), "rldm_rng_philox")
    return out.cpu().numpy().view(np.uint32)


def dev_normals(words):
    w = T(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.empty(w.shape, device="cuda", dtype=torch.float32)
    _lib.check(_lib.lib().rldm_rng_normals_from_bits(p(w), w.shape[0], p(out), _lib.stream_ptr(w.device)), "rldm_rng_normals_from_bits")
    return out.cpu().numpy()


def test_philox_on_the_device():
    kat = np.array([[0] * 4, [0xFFFFFFFF] * 4], dtype=np.uint32)
    assert [int(v) for v in dev_philox(kat[:1], (0, 0))[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in dev_philox(kat[1:], (0xFFFFFFFF, 0xFFFFFFFF))[0]] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    i = np.arange(4096, dtype=np.uint64)
    ctr = np.stack([(0x80000000 | (i * m)) & 0xFFFFFFFF for m in (2654435761, 40503, 2246822519, 3266489917)], axis=1).astype(np.uint32)
    ctr[::2] ^= np.uint32(0x7FFFFFFF)                      # high bit set in every word of the odd rows, mixed in the even ones
    assert (ctr[1::2] >> 31).all()
    key = (0x9E3779B9, 0xF0000001)
    assert np.array_equal(dev_philox(ctr, key), rng.philox_host(ctr, key))


Y_EDGES = [0, 0x100, 0x1FFFFFFF, 0x20000000, 0x3FFFFFFF, 0x40000000, 0x60000000, 0x7FFFFFFF, 0x80000000, 0xA0000000, 0xC0000000,
           0xE0000000, 0xFFFFFFFF]


def x_edges():
    """x whose u1 = ((x >> 9) + 0.5) 2^-23 sits either side of every frexp exponent change (k = 2^j - 1, 2^j) and of the sqrt(1/2)
    switch of the mantissa in every binade, exponents 0 .. -24; and the four corner words."""
    ks = {0, 1, (1 << 23) - 1}
    for j in range(0, 23):
        ks |= {(1 << j) - 1, 1 << j}
        mid = int(0.70710678 * (1 << (j + 1)) - 0.5)       # m = (k + 0.5) / 2^(j + 1) crosses fp32(0.70710678) here
        ks |= {k for k in range(mid - 2, mid + 3) if 0 <= k < (1 << 23)}
    xs = {0, 0x1FF, 0x200, 0xFFFFFFFF}
    for k in ks:
        xs |= {k << 9, (k << 9) | 0x1FF}
    return sorted(xs)


def test_transform_on_chosen_bits_is_the_host_statement_bit_for_bit():
    xs, ys = np.array(x_edges(), dtype=np.uint32), np.array(Y_EDGES, dtype=np.uint32)
    assert {0, 0x1FF, 0x200, 0xFFFFFFFF} <= set(int(v) for v in xs)
    # the sqrt(1/2) switch is taken on both sides in every binade the list covers
    u1, _ = rng.uniforms_from_bits(xs, xs)
    m, e = np.frexp(u1)
    assert set(int(v) for v in e) == set(range(-23, 1))
    for ee in range(-21, 1):                               # (the binades below hold one or two values of u1)
        mm = m[e == ee]
        assert (mm < np.float32(0.70710678)).any() and (mm >= np.float32(0.70710678)).any(), ee
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    edge = np.stack([gx.ravel(), gy.ravel(), gx.ravel()[::-1], gy.ravel()[::-1]], axis=1)
    i = np.arange(65536, dtype=np.uint64)
    sweep = np.stack([(i * 65537) & 0xFFFFFFFF, (i * 2654435761) & 0xFFFFFFFF, (i * 65521 * 65536 + 0x1FF) & 0xFFFFFFFF,
                      (i * 0x01000193 * 257) & 0xFFFFFFFF], axis=1).astype(np.uint32)
    for name, words in (("edges", edge), ("sweep", sweep)):
        got, want = dev_normals(words), rng.normals_from_bits_host(words)
        assert np.isfinite(want).all() and float(np.abs(want).max()) <= 5.77
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} normals differ; first words {words[np.nonzero(bad)[0][0]]}"


# ---- randn ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,per", [(1, 1), (1, 3), (3, 5), (2, 4097), (16, 16384)])
def test_randn_is_randn_host_bit_for_bit(B, per):
    g = rng.DeviceGenerator(SEED)
    cases = [dict(draw=0, purpose=0, row=0, sample_offset=0), dict(draw=5, purpose=1, row=(1 << 31) + 1, sample_offset=7),
             dict(draw=(1 << 30) - 1, purpose=3, row=2, sample_offset=0)]
    if B == 3:
        cases.append(dict(draw=1, purpose=2, row=9, sample_offset=(1 << 32) - 3))
    for c in cases:
        addr = g.at(c["draw"], c["purpose"], c["row"])
        got = rng.randn((B, per), addr, c["sample_offset"])
        again = rng.randn((B, per), addr, c["sample_offset"])
        want = rng.randn_host((B, per), SEED, **c)
        assert got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
        assert same(got, again), c
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), c
    assert g.draw == 0                                       # addresses consume nothing ...
    a = rng.randn((B, per), g)
    assert g.draw == 1 and np.array_equal(a.cpu().numpy(), rng.randn_host((B, per), SEED, draw=0))     # ... the generator does
    b = rng.randn((B, per), g, purpose=1, row=4, sample_offset=2)
    assert g.draw == 2 and np.array_equal(b.cpu().numpy(), rng.randn_host((B, per), SEED, 1, 1, 4, 2))


def test_randn_into_an_unaligned_view_and_through_randn_tensor():
    """A [B, per] block at an odd float offset (16-byte stores impossible), written in place without touching its neighbours; and
    schedulers.randn_tensor with a DeviceGenerator, which is rng.randn."""
    buf = torch.full((3 + 2 * 8 + 5,), 7.0, device="cuda")
    view = buf[3:19].view(2, 8)
    rng.randn((2, 8), rng.DeviceGenerator(3).at(2, 1, 5), sample_offset=4, out=view)
    want = rng.randn_host((2, 8), 3, 2, 1, 5, 4)
    assert np.array_equal(view.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((buf[:3] == 7).all()) and bool((buf[19:] == 7).all())
    g = rng.DeviceGenerator(11)
    x = randn_tensor((2, 3, 5), generator=g, device="cuda", dtype=torch.float32)
    assert g.draw == 1 and np.array_equal(x.cpu().numpy(), rng.randn_host((2, 3, 5), 11))
    t = torch.Generator().manual_seed(4)
    assert torch.equal(randn_tensor((2, 3), generator=t), torch.randn((2, 3), generator=torch.Generator().manual_seed(4)))


# ---- the captured samplers ------------------------------------------------------------------------------------------------
def explicit(gen, draw, rows, shape, offset, purposes=(1,)):
    """x_T and the [rows, *shape] tensors of `purposes` that a sampler drawing (gen.seed, draw) at `offset` reads."""
    return rng.randn(shape, gen.at(draw), offset), [rng.randn_rows(rows, shape, gen, draw, q, offset) for q in purposes]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("flags", [0, int(_lib.Flag.SCHED_LAUNCH)])
def test_ddpm_sampler_drawing_in_its_graph_equals_the_explicit_entry_point(flags, lanes, monkeypatch):
    """12 steps = two replays of a 6-step graph; B = 4 as one chain and as two lanes of 2 (the smallest split
    tests/test_hip_models.py's chain test uses); the scheduler step in conv_out's epilogue (step word -1, advanced by the step's
    first launch) and as a launch of its own (step word 0, advanced after it)."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    monkeypatch.setenv("RLDM_LANES", str(lanes))
    B, steps, offset = 4, 12, 5
    shape = (B, *LAT)
    pipe = LDMPipelineRange(vae=hip_vae(), unet=hip_unet(small_cfg(5, 4), "rng/small."), scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    fs = pipe._fused
    h = fs.get(pipe.unet, pipe.vae, pipe.scheduler, B, steps, _lib.RLDM_SAMPLER_DDPM, True, 0, plan_flags=flags)
    gen = rng.DeviceGenerator(SEED)

    def run_rng(draw, x_T=None):
        img, lat = torch.empty((B, 2, 128, 32), device="cuda"), torch.empty(shape, device="cuda")
        fs.run_rng(h, x_T, gen.seed, draw, offset, None, img, latents_out=lat)
        return img, lat

    def run_explicit(x_T, zs):
        img, lat = torch.empty((B, 2, 128, 32), device="cuda"), torch.empty(shape, device="cuda")
        fs.run(h, x_T, zs, None, img, latents_out=lat)
        return img, lat

    a0 = run_rng(0)
    caps = fs.captures(h)
    assert caps >= lanes                                     # one step graph per lane (more only if the plans were rebuilt)
    a1 = run_rng(1)
    given = T(normal(7, "rng/xT", shape)).cuda()
    a2 = run_rng(1, given)                                   # x_T given: only the step noise is drawn
    assert fs.captures(h) == caps                            # another draw, another x_T: the same graphs
    assert all(torch.isfinite(t).all() for t in a0 + a1 + a2)
    assert not same(a0[1], a1[1]) and not same(a1[1], a2[1])
    for draw, got, x_given in ((0, a0, None), (1, a1, None), (1, a2, given)):
        x_T, (zs,) = explicit(gen, draw, steps, shape, offset)
        want = run_explicit(x_given if x_given is not None else x_T, zs)
        assert same(got[1], want[1]) and same(got[0], want[0]), (draw, x_given is not None)


@pytest.mark.parametrize("mode", ["ddim", "ddpm"])
def test_guided_sampler_drawing_in_its_graph_equals_the_explicit_entry_point(mode):
    """jump_length 2, jump_n_sample 2 on 6 steps: 10 rows, known-region noise on every row but the last, re-noise on two."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    B, offset = 2, (1 << 32) - 2
    shape = (B, *LAT)
    sch = (DDIMSchedulerHIP if mode == "ddim" else DDPMSchedulerHIP)()
    pipe = LDMPipelineRange(vae=hip_vae(), unet=hip_unet(small_cfg(5, 4), "rng/small."), scheduler=sch, pos_encoding=True)
    fs = pipe._fused
    ts, tab = repaint_program(sch, 6, 2, 2)
    rows = len(ts)
    assert rows == 10 and (tab[:, 6] != 0).sum() == rows - 1 and (tab[:, 8] != 0).sum() == 2
    smode = _lib.RLDM_SAMPLER_DDIM if mode == "ddim" else _lib.RLDM_SAMPLER_DDPM
    h = fs.get(pipe.unet, pipe.vae, sch, B, rows, smode, True, 0, program=(ts, tab))
    z0 = T(normal(8, "rng/z0", shape)).cuda()
    mask = torch.ones((B, 1, 32, 8), device="cuda")
    mask[:, :, 6:20] = 0
    gen = rng.DeviceGenerator(SEED + 1)
    outs = {}
    for draw in (3, 4):
        lat = torch.empty(shape, device="cuda")
        img = torch.empty((B, 2, 128, 32), device="cuda")
        fs.run_guided_rng(h, None, gen.seed, draw, offset, z0, mask, img, latents_out=lat)
        outs[draw] = (img, lat)
        if draw == 3:
            caps = fs.captures(h)
    assert fs.captures(h) == caps
    assert not same(outs[3][1], outs[4][1])
    sel = mask.expand(shape) == 1
    for draw in (3, 4):
        x_T, (zs, nk, nr) = explicit(gen, draw, rows, shape, offset, purposes=(1, 2, 3))
        lat, img = torch.empty(shape, device="cuda"), torch.empty((B, 2, 128, 32), device="cuda")
        fs.run_guided(h, x_T, zs if mode == "ddpm" else None, z0, mask, nk, nr, img, latents_out=lat)
        assert torch.isfinite(img).all()
        assert same(outs[draw][1], lat) and same(outs[draw][0], img), draw
        assert same(lat[sel], z0[sel])                       # the known latent pixels come back bit for bit
    # x_T given
    given = T(normal(9, "rng/xT", shape)).cuda()
    lat_a, lat_b = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    fs.run_guided_rng(h, given, gen.seed, 4, offset, z0, mask, None, latents_out=lat_a)
    _, (zs, nk, nr) = explicit(gen, 4, rows, shape, offset, purposes=(1, 2, 3))
    fs.run_guided(h, given, zs if mode == "ddpm" else None, z0, mask, nk, nr, None, latents_out=lat_b)
    assert same(lat_a, lat_b) and not same(lat_a, outs[4][1])


def test_entry_points_refuse_what_the_contract_excludes():
    from rangeldm_amd.pipelines import LDMPipelineRange
    pipe = LDMPipelineRange(vae=hip_vae(), unet=hip_unet(small_cfg(5, 4), "rng/small."), scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    fs = pipe._fused
    h = fs.get(pipe.unet, pipe.vae, pipe.scheduler, 2, 2, _lib.RLDM_SAMPLER_DDPM, True, 0)
    lat = torch.empty((2, *LAT), device="cuda")
    with pytest.raises(RuntimeError, match="2\\^30"):
        fs.run_rng(h, None, 1, 1 << 30, 0, None, None, latents_out=lat)
    with pytest.raises(RuntimeError, match="2\\^32"):
        fs.run_rng(h, None, 1, 0, (1 << 32) - 1, None, None, latents_out=lat)
    with pytest.raises(RuntimeError, match="guided = 1"):
        fs.run_guided_rng(h, None, 1, 0, 0, lat, lat, None, latents_out=lat)
    with pytest.raises(RuntimeError, match="step_noise"):   # the existing entry point keeps its own refusal
        fs.run(h, lat, None, None, None, latents_out=lat)


# ---- pipelines ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_pipelines_with_a_device_generator_equal_their_explicit_twins(fused, golden):
    from rangeldm_amd.encoders import SparseRangeImageEncoder2
    from rangeldm_amd.pipelines import DDPMPipelineRange, LDMPipelineRange, LDMUpscalePipelineRange
    B, steps, offset = 2, 4, 6
    kw = dict(batch_size=B, num_inference_steps=steps, output_type="torch", fused=fused)
    vae = hip_vae()
    # pixel-space DDPM: draw 0, then draw 1 of the same generator
    pipe = DDPMPipelineRange(unet=hip_unet(small_cfg(3, 3), "rng/px."), scheduler=DDPMSchedulerHIP())
    gen = rng.DeviceGenerator(SEED)
    for draw in (0, 1):
        got = pipe(generator=gen, sample_offset=offset, **kw)
        x_T, (zs,) = explicit(gen, draw, steps, (B, 3, 32, 8), offset)
        assert gen.draw == draw + 1 and torch.isfinite(got).all()
        assert same(got, pipe(latents=x_T, step_noise=zs, **kw)), draw
    mine = T(normal(3, "rng/px/xT", (B, 3, 32, 8))).cuda()          # explicit latents keep priority; the step noise is still drawn
    _, (zs,) = explicit(gen, 2, steps, (B, 3, 32, 8), offset)
    assert same(pipe(generator=gen, sample_offset=offset, latents=mine, **kw), pipe(latents=mine, step_noise=zs, **kw))
    # latent DDPM
    shape = (B, *LAT)
    unet = hip_unet(small_cfg(5, 4), "rng/small.")
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    gen = rng.DeviceGenerator(SEED)
    got = pipe(generator=gen, sample_offset=offset, **kw)
    x_T, (zs,) = explicit(gen, 0, steps, shape, offset)
    assert same(got, pipe(latents=x_T, step_noise=zs, **kw))
    # conditional
    g = golden("up")
    up = LDMUpscalePipelineRange(vae=vae, unet=hip_unet(small_cfg(12, 4), "rng/up."), scheduler=DDPMSchedulerHIP())
    ckw = dict(image=T(g["up_cond"]).cuda(), condition_encoder=SparseRangeImageEncoder2(), **kw)
    gen = rng.DeviceGenerator(SEED)
    got = up(generator=gen, sample_offset=offset, **ckw)
    x_T, (zs,) = explicit(gen, 0, steps, shape, offset)
    assert gen.draw == 1 and same(got, up(latents=x_T, step_noise=zs, **ckw))
    # DDIM and DPM-Solver++ draw only x_T
    for sch in (DDIMSchedulerHIP(), DPMSolverMultistepSchedulerHIP()):
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=sch, pos_encoding=True)
        gen = rng.DeviceGenerator(SEED)
        got = pipe(generator=gen, sample_offset=offset, **kw)
        assert gen.draw == 1 and same(got, pipe(latents=rng.randn(shape, gen.at(0), offset), **kw)), type(sch).__name__


@pytest.mark.parametrize("fused", [True, False])
def test_guided_pipelines_with_a_device_generator_equal_their_explicit_twins(fused):
    from rangeldm_amd.pipelines import DDIMPipelineRange, LDMPipelineRange
    B, offset = 2, 3
    vae = hip_vae()
    # latent, DDPM rows: all three purposes
    pipe = LDMPipelineRange(vae=vae, unet=hip_unet(small_cfg(5, 4), "rng/small."), scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    rows = len(repaint_program(pipe.scheduler, 6, 2, 2)[0])
    known = T(normal(4, "rng/known", (B, 2, 128, 32))).cuda() * 0.5
    mask = torch.ones((B, 1, 128, 32), device="cuda")
    mask[:, :, 20:52] = 0
    kw = dict(batch_size=B, num_inference_steps=6, known=known, known_mask=mask, jump_length=2, jump_n_sample=2, output_type="torch",
              return_latents=True, fused=fused)
    gen = rng.DeviceGenerator(SEED)
    img, lat, z0, lat_mask = pipe(generator=gen, sample_offset=offset, **kw)
    x_T, (zs, nk, nr) = explicit(gen, 0, rows, (B, *LAT), offset, purposes=(1, 2, 3))
    img2, lat2, _, _ = pipe(latents=x_T, step_noise=zs, known_noise=nk, renoise_noise=nr, **kw)
    assert gen.draw == 1 and torch.isfinite(img).all() and same(lat, lat2) and same(img, img2)
    sel = lat_mask.expand_as(lat) == 1
    assert 0 < int(sel.sum()) < sel.numel() and same(lat[sel], z0[sel])
    # one explicit tensor keeps priority; the others are still the generator's rows
    mine = T(normal(5, "rng/nk", (rows, B, *LAT))).cuda()
    _, lat3, _, _ = pipe(generator=rng.DeviceGenerator(SEED), sample_offset=offset, known_noise=mine, **kw)
    _, lat4, _, _ = pipe(latents=x_T, step_noise=zs, known_noise=mine, renoise_noise=nr, **kw)
    assert same(lat3, lat4) and not same(lat3, lat)
    # pixel space, DDIM rows
    px = DDIMPipelineRange(unet=hip_unet(UNetConfig(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64)), "rng/gpx."),
                           scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    shape = (B, 4, 64, 8)
    z0 = T(normal(6, "rng/px/z0", shape)).cuda()
    pmask = torch.ones((B, 1, 64, 8), device="cuda")
    pmask[:, :, 8:40] = 0
    pmask[1, :, :, ::2] = 0
    pkw = dict(batch_size=B, num_inference_steps=4, known=z0, known_mask=pmask, jump_length=2, jump_n_sample=2, output_type="torch", fused=fused)
    prow = len(repaint_program(px.scheduler, 4, 2, 2)[0])
    gen = rng.DeviceGenerator(SEED)
    out = px(generator=gen, sample_offset=offset, **pkw)
    x_T, (nk, nr) = explicit(gen, 0, prow, shape, offset, purposes=(2, 3))
    assert same(out, px(latents=x_T, known_noise=nk, renoise_noise=nr, **pkw))
    psel = pmask.expand(shape) == 1
    assert same(out[psel], z0[psel])


def test_a_torch_generator_gives_what_it_gave():
    """The torch path, reconstructed draw by draw through the functions it always used: x_T on the CPU, then one randn per row with
    t > 0 on the device's generator order (_draw_step_noise) -- and the call with generator= equals the call with those tensors."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    B, steps = 2, 4
    pipe = LDMPipelineRange(vae=hip_vae(), unet=hip_unet(small_cfg(5, 4), "rng/small."), scheduler=DDPMSchedulerHIP(), pos_encoding=True)
    kw = dict(batch_size=B, num_inference_steps=steps, output_type="torch")
    got = pipe(generator=torch.Generator().manual_seed(5), **kw)
    g = torch.Generator().manual_seed(5)
    x_T = randn_tensor((B, *LAT), generator=g)
    pipe.scheduler.set_timesteps(steps)
    zs = pipe._draw_step_noise(steps, pipe.scheduler.timesteps, (B, *LAT), g, pipe.device)
    assert same(got, pipe(latents=x_T, step_noise=zs, **kw))
    assert torch.equal(x_T, torch.randn((B, *LAT), generator=torch.Generator().manual_seed(5)))


def test_the_noise_of_a_sample_does_not_depend_on_the_batch():
    """B = 4 at offset 10 against two draws of B = 2 at offsets 10 and 12 (two ranks' shares), and against the host."""
    whole = rng.randn((4, *LAT), rng.DeviceGenerator(SEED).at(0), 10)
    parts = torch.cat([rng.randn((2, *LAT), rng.DeviceGenerator(SEED).at(0), 10 + o) for o in (0, 2)])
    assert same(whole, parts)
    assert np.array_equal(whole.cpu().numpy(), rng.randn_host((4, *LAT), SEED, sample_offset=10))


# ---- trainers -------------------------------------------------------------------------------------------------------------
def test_unet_training_step_with_a_device_generator_equals_the_host_statement():
    from rangeldm_amd import training as TR
    cfg = small_cfg(5, 4)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="rng/tr.")
    sch = DDPMSchedulerHIP()
    B, offset = 2, 40
    lat = T(normal(12, "rng/tr/lat", (B, *LAT)))
    runs = []
    for explicit_twin in (False, True):
        tr = TR.UNetTrainer(cfg, sd, use_ema=False, deterministic=True)
        gen = rng.DeviceGenerator(SEED)
        losses = []
        for step in range(2):
            if explicit_twin:
                noise = T(rng.randn_host((B, *LAT), SEED, draw=step, sample_offset=offset)).cuda()
                t = T(rng.timesteps_host(B, SEED, step, sch.config.num_train_timesteps, offset))
                assert t.dtype == torch.int64 and 0 <= int(t.min()) and int(t.max()) < sch.config.num_train_timesteps
                losses.append(float(TR.training_step(tr, None, sch, lat, noise=noise, timesteps=t)))
            else:
                losses.append(float(TR.training_step(tr, None, sch, lat, generator=gen, sample_offset=offset)))
        if not explicit_twin:
            assert gen.draw == 2
        torch.cuda.synchronize()
        runs.append((losses, tr.params.clone()))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(runs[0][0]))
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1]))


def test_vae_train_step_with_a_device_generator_equals_the_host_statement():
    from rangeldm_amd.vae_training import VAETrainer
    from tests.test_vae_training_gpu import SMALL
    cfg = SMALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    B, f, offset = 2, cfg.downscale, 9
    images = torch.rand(B, cfg.in_channels, *cfg.sample_size, generator=torch.Generator().manual_seed(3))
    zshape = (B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f)
    runs = []
    for explicit_twin in (False, True):
        tr = VAETrainer(cfg, sd, lr=1e-3, deterministic=True)
        gen = rng.DeviceGenerator(SEED)
        losses = []
        for step in range(2):
            if explicit_twin:
                noise = T(rng.randn_host(zshape, SEED, draw=step, sample_offset=offset)).cuda()
                losses.append(float(tr.train_step(images.cuda(), noise=noise)))
            else:
                losses.append(float(tr.train_step(images.cuda(), generator=gen, sample_offset=offset)))
        runs.append((losses, tr.params.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(bits(runs[0][1]), bits(runs[1][1]))


# ---- drivers --------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _npys(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_device_rng_driver_repeats_byte_for_byte(tmp_path):
    from rangeldm_amd import inference
    args = ["--cfg", "RangeLDM", "--samples", "3", "--batch_size", "2", "--steps", "2", "--save-npy", "--device-rng"]
    for k in ("a", "b"):
        inference.main(args + ["--out", str(tmp_path / k)])
    a, b = _npys(tmp_path / "a"), _npys(tmp_path / "b")
    assert sorted(a) == sorted(b) and len(a) == 3 * 4 and a == b
    inference.main(args[:-1] + ["--out", str(tmp_path / "c")])       # without the flag: other noise, the same file set
    c = _npys(tmp_path / "c")
    assert sorted(c) == sorted(a) and c["0.npy"] != a["0.npy"]


def test_device_rng_driver_writes_the_same_images_from_one_and_from_two_ranks(tmp_path):
    """python -m rangeldm_amd.inference --device-rng with 1 rank and with 2 ranks on one GPU over gloo (persistent launches off, as
    tests/test_bench_cli.py runs two ranks on one device): every image index gets the same bytes, so it got the same noise."""
    env = dict(os.environ, RLDM_DIST_BACKEND="gloo", RLDM_DBG_FLAGS=str(1 << 24), HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for nproc in (1, 2):
        out = tmp_path / f"w{nproc}"
        launcher = ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
                     "127.0.0.1", "--master-port", str(_free_port())] if nproc > 1 else [sys.executable])
        r = subprocess.run(launcher + ["-m", "rangeldm_amd.inference", "--cfg", "RangeLDM", "--samples", "4", "--batch_size", "2", "--steps",
                                       "2", "--save-npy", "--device-rng", "--out", str(out)], capture_output=True, text=True, timeout=300,
                           cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[nproc] = {n: v for n, v in _npys(out).items() if n.endswith(".npy")}
    assert sorted(outs[1]) == [f"{i}.npy" for i in range(4)] and outs[1] == outs[2]
