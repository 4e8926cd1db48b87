"""GPU: guided sampling on unconditional weights -- rldm_sched_guided_step exactly (against rldm_sched_step, against the fp32 blend
restated on the host, pixel by pixel under a checkerboard mask), the guided captured loop against the unguided one, against the
row-by-row loop and against a loop built from the oracle's UNet and scheduler, the rldm_sampler_status contract, and the drivers."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd.config import SchedulerConfig, UNetConfig, VAEConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.schedulers import DDIMSchedulerHIP, DDPMSchedulerHIP, guided_step, repaint_program
from rangeldm_amd.synth import normal, synth_state_dict
from oracle import pipelines as o_pipe, schedulers as o_sched, unet as o_unet
from tests.hip_util import rel_l2

pytestmark = pytest.mark.gpu
TOL_FWD = 1.2e-2     # one network forward, teacher-forced (tests/test_hip_models.py)
PTYPES = ("epsilon", "v_prediction", "sample")
MODES = ("ddim", "ddpm")
SHAPES = ((2, 4, 32, 8), (1, 3, 5, 7))       # float4 path; a shape no vector load fits
SMALL = dict(sample_size=(64, 8), block_out_channels=(32, 32, 64, 64))


def T(a):
    return torch.from_numpy(np.asarray(a))


def make_sched(mode, ptype="epsilon"):
    return (DDIMSchedulerHIP if mode == "ddim" else DDPMSchedulerHIP)(SchedulerConfig(prediction_type=ptype))


def hip_unet(cfg, prefix):
    from rangeldm_amd.unet import UNet2DModelHIP
    sd = synth_state_dict(unet_param_shapes(cfg), prefix=prefix)
    m = UNet2DModelHIP(cfg)
    m.load_state_dict(sd)
    return m, sd


_VAE = {}


def hip_vae():
    from rangeldm_amd.vae import AutoencoderKLHIP
    if "m" not in _VAE:
        sd = synth_state_dict(vae_param_shapes(VAEConfig()), prefix="vae.")
        m = AutoencoderKLHIP(VAEConfig())
        m.load_state_dict(sd)
        _VAE["m"] = m
    return _VAE["m"]


def operands(seed, shape):
    return {k: T(normal(seed, f"guided/{k}", shape)).cuda() for k in ("out", "x", "noise", "z0", "nk", "nr")}


def a_row(sch, n=10, jump=False):
    """A middle row of a program (sigma != 0 for DDPM, kb != 0); jump: one that re-noises."""
    ts, tab = repaint_program(sch, n, 2, 2)
    i = int(np.nonzero(tab[:, 8] != 0.0)[0][0]) if jump else 1
    assert tab[i, 6] != 0.0 and (tab[i, 8] != 0.0) == jump
    return int(ts[i]), tab[i].copy()


# ---- the stand-alone step, exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_unknown_everywhere_is_the_scheduler_step_bit_for_bit(mode, ptype, shape):
    sch = make_sched(mode, ptype)
    t, row = a_row(sch)
    row[7:] = (1.0, 0.0)
    o = operands(91, shape)
    mask = torch.zeros((shape[0], 1, *shape[2:]), device="cuda")
    nz = o["noise"] if row[4] != 0.0 else None
    assert (mode == "ddpm") == (nz is not None)
    want = sch._launch(0 if mode == "ddim" else 1, row[:5], o["out"], o["x"], nz)
    z0 = torch.full_like(o["z0"], float("nan"))                    # an unknown pixel does not read z0 either
    got = guided_step(sch, row, o["out"], o["x"], nz, z0, mask, o["nk"], None)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_known_everywhere_is_the_host_expression_and_ignores_the_model(mode, shape):
    sch = make_sched(mode)
    t, row = a_row(sch)
    row[7:] = (1.0, 0.0)
    o = operands(92, shape)
    mask = torch.ones((shape[0], 1, *shape[2:]), device="cuda")
    nz = o["noise"] if row[4] != 0.0 else None
    got = guided_step(sch, row, o["out"], o["x"], nz, o["z0"], mask, o["nk"], None).cpu().numpy()
    ka, kb = np.float32(row[5]), np.float32(row[6])
    z0, nk = o["z0"].cpu().numpy(), o["nk"].cpu().numpy()
    a = (ka * z0).astype(np.float32)                               # numpy: one rounding per operation, nothing fused
    b = (kb * nk).astype(np.float32)
    want = (a + b).astype(np.float32)
    assert got.view(np.int32).tobytes() == want.view(np.int32).tobytes()
    for bad in (float("inf"), float("nan")):
        poisoned = guided_step(sch, row, torch.full_like(o["out"], bad), o["x"], nz, o["z0"], mask, o["nk"], None).cpu().numpy()
        assert poisoned.view(np.int32).tobytes() == want.view(np.int32).tobytes()
    # the last row of a program: (ka, kb) = (1, 0) returns z0 itself, and no known_noise tensor is needed
    last = row.copy()
    last[5:7] = (1.0, 0.0)
    out = guided_step(sch, last, o["out"], o["x"], nz, o["z0"], mask, None, None)
    assert torch.equal(out.view(torch.int32), o["z0"].view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_checkerboard_mask_selects_per_pixel(mode, ptype, shape):
    sch = make_sched(mode, ptype)
    t, row = a_row(sch)
    row[7:] = (1.0, 0.0)
    o = operands(93, shape)
    B, Cc, W, H = shape
    w, h = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="ij")
    board = ((w + h) % 2).float()
    mask = torch.stack([board if b % 2 == 0 else 1 - board for b in range(B)])[:, None].cuda().contiguous()
    nz = o["noise"] if row[4] != 0.0 else None
    zeros, ones = torch.zeros_like(mask), torch.ones_like(mask)
    unknown = guided_step(sch, row, o["out"], o["x"], nz, o["z0"], zeros, o["nk"], None)
    known = guided_step(sch, row, o["out"], o["x"], nz, o["z0"], ones, o["nk"], None)
    got = guided_step(sch, row, o["out"], o["x"], nz, o["z0"], mask, o["nk"], None)
    want = torch.where(mask.expand(shape) == 1, known, unknown)
    assert not torch.equal(known, unknown)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # in place (x_prev == x), as the captured loop runs it
    x = o["x"].clone()
    cf = (C.c_float * 9)(*[float(v) for v in row])

    def p(t_):
        return C.c_void_p(t_.data_ptr()) if t_ is not None else None
    _lib.check(_lib.lib().rldm_sched_guided_step(0 if mode == "ddim" else 1, sch.prediction_code, cf, p(o["out"]), p(x), p(nz), p(o["z0"]),
                                                 p(mask), p(o["nk"]), None, p(x), B, Cc, W * H, _lib.stream_ptr(x.device)), "in place")
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES)
def test_renoise_and_fractional_mask_match_fp64(shape):
    sch = make_sched("ddpm")
    t, row = a_row(sch, jump=True)
    o = operands(94, shape)
    mask = T(normal(94, "guided/m", (shape[0], 1, *shape[2:]))).cuda().sigmoid()
    mask[..., 0] = 1.0
    mask[..., 1] = 0.0
    got = guided_step(sch, row, o["out"], o["x"], o["noise"], o["z0"], mask, o["nk"], o["nr"]).cpu().double()
    c = row.astype(np.float64)
    d = {k: v.cpu().double() for k, v in o.items()}
    x0 = (d["x"] - c[1] * d["out"]) / c[0]
    u = c[2] * x0 + c[3] * d["x"] + c[4] * d["noise"]
    m = mask.cpu().double()
    g = m * (c[5] * d["z0"] + c[6] * d["nk"]) + (1 - m) * u
    want = c[7] * g + c[8] * d["nr"]
    assert (got - want).abs().max() < 2e-5 * (1 + want.abs().max())
    with pytest.raises(RuntimeError, match="renoise_noise"):
        guided_step(sch, row, o["out"], o["x"], o["noise"], o["z0"], mask, o["nk"], None)


# ---- the captured loop ------------------------------------------------------------------------------------------------------
def guided_run(pipe, vae, unet, x_T, program, zs, z0, mask, nk, nr, image_shape=None):
    B = x_T.shape[0]
    mode = 0 if isinstance(pipe.scheduler, DDIMSchedulerHIP) else 1
    h = pipe._fused.get(unet, vae, pipe.scheduler, B, len(program[0]), mode, pipe.pos_encoding, 0, program=program)
    lat = torch.empty_like(x_T)
    img = torch.empty(image_shape, device="cuda") if image_shape else None
    pipe._fused.run_guided(h, x_T, zs, z0, mask, nk, nr, img, latents_out=lat)
    return lat, img, h


@pytest.mark.parametrize("size", ["reduced", "headline"])
@pytest.mark.parametrize("mode", MODES)
def test_unknown_everywhere_matches_the_unguided_separate_launch_sampler(mode, size):
    """mask == 0, no resampling: the guided sampler against an unguided one whose scheduler step is a launch of its own
    (Flag.SCHED_LAUNCH).  The parent's tests hold that route to rel-L2 < 1e-5 of the fused tail (tests/test_dpmsolver_gpu.py), not
    to bit-equality, so that is the gate here; the kernel-level tests above are the exact ones."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    if size == "reduced":
        cfg, prefix, lat_shape = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64)), \
            "guided/small.", (2, 4, 32, 8)
    else:
        cfg, prefix, lat_shape = UNetConfig(), "", (2, 4, 256, 16)
    unet, _ = hip_unet(cfg, prefix)
    vae = hip_vae()
    n = 4
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_sched(mode), pos_encoding=True)
    x_T = T(normal(95, "guided/xT", lat_shape)).cuda()
    zs = T(normal(95, "guided/zs", (n, *lat_shape))).cuda() if mode == "ddpm" else None
    img_shape = (lat_shape[0], 2, lat_shape[2] * 4, lat_shape[3] * 4)
    h = pipe._fused.get(unet, vae, pipe.scheduler, lat_shape[0], n, 0 if mode == "ddim" else 1, True, 0, plan_flags=_lib.Flag.SCHED_LAUNCH)
    want_img, want_lat = torch.empty(img_shape, device="cuda"), torch.empty_like(x_T)
    pipe._fused.run(h, x_T, zs, None, want_img, latents_out=want_lat)
    program = repaint_program(pipe.scheduler, n)
    z0 = torch.full_like(x_T, float("nan"))
    mask = torch.zeros((lat_shape[0], 1, *lat_shape[2:]), device="cuda")
    nk = T(normal(95, "guided/nk", (n, *lat_shape))).cuda()           # (asked for because kb != 0; no pixel is known, so never used)
    lat, img, _ = guided_run(pipe, vae, unet, x_T, program, zs, z0, mask, nk, None, img_shape)
    assert torch.isfinite(want_img).all() and torch.isfinite(img).all()
    e_lat, e_img = rel_l2(lat, want_lat), rel_l2(img, want_img)
    print(f"guided (mask 0) vs unguided separate-launch sampler, {mode} {size}: latent rel-L2 {e_lat:.3e}, image {e_img:.3e}, "
          f"bit-equal {torch.equal(lat, want_lat) and torch.equal(img, want_img)}")
    assert e_lat < 1e-5 and e_img < 1e-5


def span_mask(B, W, H, w0, w1):
    m = torch.ones((B, 1, W, H))
    m[:, :, w0:w1] = 0
    return m


@pytest.mark.parametrize("mode", MODES)
def test_captured_loop_matches_row_by_row_loop_with_jumps(mode):
    """jump_length 2, jump_n_sample 2 on 6 steps, all three noise tensors injected: LDMPipelineRange fused against fused=False (every
    row through unet(...) and rldm_sched_guided_step), held to what the fused-vs-unfused DDPM tests hold (rel-L2 < 1e-5); and the
    known latent pixels of the result are z0, bit for bit."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64))
    unet, _ = hip_unet(cfg, "guided/small.")
    vae = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_sched(mode), pos_encoding=True)
    ts, tab = repaint_program(pipe.scheduler, 6, 2, 2)
    rows = len(ts)
    assert rows == 6 + 2 * 2 and (tab[:, 8] != 0).sum() == 2
    shape = (2, 4, 32, 8)
    x_T = T(normal(96, "guided/xT", shape))
    zs, nk, nr = (T(normal(96, f"guided/{k}", (rows, *shape))).cuda() for k in ("zs", "nk", "nr"))
    known = T(normal(96, "guided/known", (2, 2, 128, 32))).cuda() * 0.5
    mask = span_mask(2, 128, 32, 20, 52).cuda()
    kw = dict(batch_size=2, num_inference_steps=6, latents=x_T, known=known, known_mask=mask, jump_length=2, jump_n_sample=2,
              known_noise=nk, renoise_noise=nr, output_type="torch", return_latents=True)
    if mode == "ddpm":
        kw["step_noise"] = zs
    img, lat, z0, lat_mask = pipe(**kw)
    img2, lat2, _, _ = pipe(fused=False, **kw)
    assert torch.isfinite(img).all() and img.shape == (2, 2, 128, 32)
    print(f"guided {mode} fused vs row by row: latent rel-L2 {rel_l2(lat, lat2):.3e}, image {rel_l2(img, img2):.3e}")
    assert rel_l2(lat, lat2) < 1e-5 and rel_l2(img, img2) < 1e-5
    sel = lat_mask.expand_as(lat) == 1
    assert 0 < int(sel.sum()) < sel.numel()
    for got in (lat, lat2):
        assert torch.equal(got[sel].view(torch.int32), z0[sel].view(torch.int32))
    assert not torch.equal(lat[~sel], z0[~sel])
    # the jumps are part of the sampler: without them the unknown region differs, the known one does not
    kw1 = dict(kw, jump_n_sample=1, known_noise=nk[:6], renoise_noise=None)
    if mode == "ddpm":
        kw1["step_noise"] = zs[:6]
    _, lat1, _, _ = pipe(**kw1)
    assert torch.equal(lat1[sel], z0[sel]) and rel_l2(lat1, lat) > 1e-3
    assert len(pipe._fused._cache) == 2


def oracle_guided_loop(ounet, osch, ts, tab, x_T, z0, mask, nk, nr, pos_encoding=True, trajectory=None):
    """The guided loop from the oracle's UNet and scheduler step plus the blend and the re-noise in torch fp32."""
    x = x_T.clone()
    pe = o_pipe.pos_encoding_channel(x.shape[0], x.shape[2], x.shape[3]) if pos_encoding else None
    for i, t in enumerate(ts):
        eps = ounet(torch.cat([x, pe], 1) if pos_encoding else x, t).sample
        if trajectory is not None:
            trajectory.append((x.clone(), eps.clone()))
        u = osch.step(eps, t, x).prev_sample
        ka, kb, ra, rb = (float(v) for v in tab[i, 5:])
        g = mask * (ka * z0 + kb * nk[i]) + (1 - mask) * u
        x = ra * g + rb * nr[i]
    return x


def test_guided_loop_matches_oracle_loop():
    """Pixel-space DDIM on the reduced UNet of tests/test_hip_models.py's captured-vs-oracle tests, 6 network evaluations (4 steps,
    one jump of length 2): teacher-forced per row (eps at the oracle's x: TOL_FWD; the guided step on the oracle's operands: the 2e-5
    of the scheduler-step tests) and free-running on the final sample (3 * TOL_FWD, the gate of
    test_captured_sampler_honours_prediction_type for this config and 6 evaluations)."""
    from rangeldm_amd.pipelines import DDIMPipelineRange
    cfg = UNetConfig(**SMALL)
    unet, sd = hip_unet(cfg, "guided/px.")
    ounet = o_unet.OracleUNet(cfg, sd)
    pipe = DDIMPipelineRange(unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=True)
    ts, tab = repaint_program(pipe.scheduler, 4, 2, 2)
    rows = len(ts)
    assert rows == 6
    shape = (2, 4, 64, 8)
    x_T, z0 = T(normal(97, "guided/xT", shape)), T(normal(97, "guided/z0", shape))
    nk, nr = (T(normal(97, f"guided/{k}", (rows, *shape))) for k in ("nk", "nr"))
    mask = span_mask(2, 64, 8, 8, 40)
    mask[1, :, :, ::2] = 0                                         # any pattern in pixel space
    osch = o_sched.OracleDDIMScheduler()
    osch.set_timesteps(4)
    traj = []
    ref = oracle_guided_loop(ounet, osch, ts, tab, x_T, z0, mask, nk, nr, trajectory=traj)
    pe = o_pipe.pos_encoding_channel(2, 64, 8)
    for i, ((x_i, eps_ref), t) in enumerate(zip(traj, ts)):
        eps = unet(torch.cat([x_i, pe], 1).cuda(), t).sample.cpu()
        assert rel_l2(eps, eps_ref) < TOL_FWD, i
        nxt = traj[i + 1][0] if i + 1 < rows else ref
        got = guided_step(pipe.scheduler, tab[i], eps_ref.cuda(), x_i.cuda(), None, z0.cuda(), mask.cuda(), nk[i].cuda(), nr[i].cuda()).cpu()
        assert (got - nxt).abs().max() < 2e-5 * (1 + nxt.abs().max()), i
    kw = dict(batch_size=2, num_inference_steps=4, latents=x_T, known=z0, known_mask=mask, jump_length=2, jump_n_sample=2,
              known_noise=nk, renoise_noise=nr, output_type="torch")
    out = pipe(**kw).cpu()
    loop = pipe(fused=False, **kw).cpu()
    e = rel_l2(out, ref)
    print(f"guided DDIM, 6 rows, free-running vs oracle loop: rel-L2 {e:.3e}; fused vs row by row {rel_l2(out, loop):.3e}")
    assert torch.isfinite(out).all() and e < 3 * TOL_FWD
    assert rel_l2(out, loop) < 1e-5
    sel = mask.expand(shape) == 1
    assert torch.equal(out[sel].view(torch.int32), z0[sel].view(torch.int32))      # known pixels: z0, bit for bit
    # drawn noise: seeded calls repeat, and the generator is used after x_T
    a = pipe(batch_size=2, num_inference_steps=4, generator=torch.Generator().manual_seed(5), known=z0, known_mask=mask, jump_length=2,
             jump_n_sample=2, output_type="torch")
    b = pipe(batch_size=2, num_inference_steps=4, generator=torch.Generator().manual_seed(5), known=z0, known_mask=mask, jump_length=2,
             jump_n_sample=2, output_type="torch")
    assert torch.equal(a, b) and torch.equal(a.cpu()[sel], z0[sel])


def test_entry_points_refuse_the_wrong_sampler_and_dpmsolver():
    from rangeldm_amd.pipelines import LDMPipelineRange
    cfg = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64))
    unet, _ = hip_unet(cfg, "guided/small.")
    vae = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_sched("ddim"), pos_encoding=True)
    program = repaint_program(pipe.scheduler, 3)
    x = torch.zeros((1, 4, 32, 8), device="cuda")
    m = torch.zeros((1, 1, 32, 8), device="cuda")
    hg = pipe._fused.get(unet, vae, pipe.scheduler, 1, 3, 0, True, 0, program=program)
    hu = pipe._fused.get(unet, vae, pipe.scheduler, 1, 3, 0, True, 0)
    with pytest.raises(RuntimeError, match="rldm_sample_guided"):
        pipe._fused.run(hg, x, None, None, None, latents_out=torch.empty_like(x))
    with pytest.raises(RuntimeError, match="guided = 1"):
        pipe._fused.run_guided(hu, x, None, x, m, None, None, None, latents_out=torch.empty_like(x))
    with pytest.raises(RuntimeError, match="known_noise"):
        pipe._fused.run_guided(hg, x, None, x, m, None, None, None, latents_out=torch.empty_like(x))
    with pytest.raises(RuntimeError, match="DPM-Solver"):
        pipe._fused.get(unet, vae, pipe.scheduler, 1, 3, _lib.RLDM_SAMPLER_DPMSOLVER, True, 0, program=program)


def test_status_contract_holds_for_a_guided_sampler():
    """tests/test_hip_models.py's mid-run failure test on a guided sampler: the call with the injected trunk error raises, its
    outputs are NaN-marked, and the next call succeeds with the images of a healthy run."""
    from rangeldm_amd.pipelines import LDMPipelineRange
    unet, _ = hip_unet(UNetConfig(), "")
    vae = hip_vae()
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_sched("ddim"), pos_encoding=True)
    x_T = T(normal(98, "guided/xT", (16, 4, 256, 16)))
    known = T(normal(98, "guided/known", (16, 2, 1024, 64))).cuda() * 0.5
    mask = span_mask(16, 1024, 64, 0, 64).cuda()
    ts, tab = repaint_program(pipe.scheduler, 2)
    nk = T(normal(98, "guided/nk", (2, 16, 4, 256, 16))).cuda()
    kw = dict(batch_size=16, num_inference_steps=2, latents=x_T, known=known, known_mask=mask, known_noise=nk, output_type="torch")
    good = pipe(**kw).cpu()
    assert torch.isfinite(good).all()
    h = pipe._fused.get(unet, vae, pipe.scheduler, 16, 2, 0, True, 0, program=(ts, tab))
    _lib.check(_lib.lib().rldm_debug_inject_trunk_error(h, 1), "inject")
    with pytest.raises(RuntimeError, match="self-check"):
        pipe(**kw)
    assert torch.equal(pipe(**kw).cpu(), good)                     # the sampler fell back by itself: identical images


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def test_guided_driver_then_evaluate_inpainting(tmp_path, capsys):
    from rangeldm_amd import evaluate, inference_conditional
    out = tmp_path / "guided"
    inference_conditional.main(["--guided", "--cfg", "RangeLDM", "--samples", "2", "--batch_size", "2", "--steps", "4",
                                "--jump-length", "2", "--jump-n-sample", "2", "--out", str(out)])
    names = sorted(p.name for p in (out / "inpainting_result").iterdir())
    assert names[:2] == ["0_seed_0.bin", "0_seed_0.png"]
    assert sorted(p.name for p in (out / "inpainting_target").iterdir()) == ["0_seed_0.bin", "0_seed_0.png", "1_seed_0.bin", "1_seed_0.png"]
    capsys.readouterr()
    evaluate.main(["inpainting", "--exp", str(out)])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["task"] == "inpainting" and res["pairs"] >= 2 and res["window"] == [0, 64]
    assert np.isfinite(res["cd"]) and np.isfinite(res["mae_m"]["per_masked_pixel"])


def test_pixel_space_driver_leaves_the_unmasked_part_untouched(tmp_path):
    """RangeDM through the driver: the MAE over the unmasked azimuth columns is exactly 0 (the known pixels are copied, not
    regenerated)."""
    from rangeldm_amd import inference_conditional
    from rangeldm_amd.metrics import range_errors
    out = tmp_path / "px"
    inference_conditional.main(["--guided", "--cfg", "RangeDM", "--samples", "1", "--batch_size", "1", "--steps", "3", "--save-npy",
                                "--out", str(out)])
    res = T(np.load(out / "inpainting_result" / "0_seed_0.npy"))[None].cuda()
    tgt = T(np.load(out / "inpainting_target" / "0_seed_0.npy"))[None].cuda()
    assert res.shape == (1, 2, 1024, 64) and torch.isfinite(res).all()
    sa, sq, count = range_errors(res, tgt, scale=[1.0, 1.0], window=(64, 1024))        # the mask is the span [0, 64)
    assert float(sa.sum()) == 0.0 and float(sq.sum()) == 0.0 and count > 0
    sa_in, _, _ = range_errors(res, tgt, scale=[1.0, 1.0], window=(0, 64))
    assert float(sa_in.sum()) > 0.0                                                       # ... and the masked span was generated
    dens = tmp_path / "dens"
    inference_conditional.main(["--guided", "--task", "densification", "--cfg", "RangeDM", "--samples", "1", "--batch_size", "1",
                                "--steps", "2", "--save-npy", "--out", str(dens)])
    res = np.load(dens / "densification_result" / "0_seed_0.npy")
    tgt = np.load(dens / "densification_target" / "0_seed_0.npy")
    assert np.array_equal(res[..., 2::4], tgt[..., 2::4]) and not np.array_equal(res, tgt)
    with pytest.raises(ValueError, match="pixel-space"):
        inference_conditional.main(["--guided", "--task", "densification", "--cfg", "RangeLDM", "--samples", "1", "--batch_size", "1",
                                    "--steps", "2", "--out", str(tmp_path / "no")])
