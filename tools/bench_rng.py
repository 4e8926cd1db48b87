#!/usr/bin/env python3
"""What the device generator (csrc/rng.hip, rangeldm_amd/rng.py) costs and saves -- three measurements in ONE process on one GPU,
the variants of each interleaved round by round so that clock and temperature drift hits them alike:

  fill     rng.randn against torch.randn on the device at batch 16, for a latent (4 x 256 x 16) and a pixel-space sample
           (2 x 1024 x 64) and for 64 of the latter stacked (a size that no cache holds): normals/s and GB/s written
  ddpm     the pixel-space ancestral sampler (RangeDM, DDPMPipelineRange, --ddpm-steps rows, batch 16): noise drawn inside the step
           graph (rldm_sample_rng) against an explicit [steps, B, 2, 1024, 64] tensor -- seconds per call and noise bytes held
  guided   tools/bench_guided.py's RePaint program (RangeLDM, 50 DDIM steps, jump 10 x 10: 410 rows, known-region and re-noise
           tensors) with and without device noise

    python tools/bench_rng.py [--only fill,ddpm,guided] [--reps 5] [--batch 16] [--ddpm-steps 1000]

One warm-up call of each variant, then --reps rounds of one timed call each (host clock around the call and a device
synchronise; `fill` times --fill-iters back-to-back launches per call).  Median [min, max] per variant.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def interleaved(cases, reps):
    """cases: name -> callable.  One warm-up each, then `reps` rounds; -> name -> [seconds]."""
    times = {k: [] for k in cases}
    for run in cases.values():
        run()
        torch.cuda.synchronize()
    for _ in range(reps):
        for k, run in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return times


def stats(ts):
    return {"seconds": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts)}


def bench_fill(a):
    from rangeldm_amd import rng
    gen = rng.DeviceGenerator(1)
    out = {}
    for name, shape in (("latent_4x256x16", (a.batch, 4, 256, 16)), ("pixel_2x1024x64", (a.batch, 2, 1024, 64)),
                        ("pixel_2x1024x64_x64", (a.batch * 64, 2, 1024, 64))):
        buf = torch.empty(shape, device="cuda")
        n = buf.numel()
        addr = gen.at(0, 1, 3)

        def ours():
            for _ in range(a.fill_iters):
                rng.randn(shape, addr, out=buf)

        def theirs():
            for _ in range(a.fill_iters):
                torch.randn(shape, device="cuda", out=buf)
        res = {}
        for k, ts in interleaved({"rng_randn": ours, "torch_randn": theirs}, a.reps).items():
            s = stats(ts)
            per = {q: v / a.fill_iters for q, v in s.items()}
            res[k] = {"us_per_fill": 1e6 * per["seconds"], "us_min": 1e6 * per["seconds_min"], "us_max": 1e6 * per["seconds_max"],
                      "normals_per_s": n / per["seconds"], "GB_per_s_written": 4 * n / per["seconds"] / 1e9}
        res["elements"] = n
        out[name] = res
    return out


def bench_ddpm(a):
    from rangeldm_amd import _lib, rng
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import unet_param_shapes
    from rangeldm_amd.pipelines import DDPMPipelineRange, _FusedSampler
    from rangeldm_amd.schedulers import DDPMSchedulerHIP
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.unet import UNet2DModelHIP
    import dataclasses
    # RangeDM's network without its position channel: DDPMPipelineRange has none (2 x 1024 x 64 in, 2 x 1024 x 64 out)
    ucfg = dataclasses.replace(PRESETS["RangeDM"]["unet"], in_channels=2)
    unet = UNet2DModelHIP(ucfg)
    unet.load_state_dict(synth_state_dict(unet_param_shapes(ucfg), prefix=""))
    pipe = DDPMPipelineRange(unet=unet, scheduler=DDPMSchedulerHIP())
    B, N = a.batch, a.ddpm_steps
    shape = (B, ucfg.in_channels, *ucfg.sample_size)
    fs = pipe._fused
    h = fs.get(unet, None, pipe.scheduler, B, N, _lib.RLDM_SAMPLER_DDPM, False, 0)
    gen = rng.DeviceGenerator(2)
    img = torch.empty(shape, device="cuda")
    x_T = rng.randn(shape, gen.at(0))
    base = torch.cuda.memory_allocated()
    zs = rng.randn_rows(N, shape, gen, 0, 1)
    explicit_bytes = torch.cuda.memory_allocated() - base
    # a sampler captures its step graph around the noise pointers it was given: one sampler per variant, so that alternating calls
    # replay their graphs instead of capturing again
    fs2 = _FusedSampler()
    h2 = fs2.get(unet, None, pipe.scheduler, B, N, _lib.RLDM_SAMPLER_DDPM, False, 0)
    times = interleaved({"device_noise": lambda: fs.run_rng(h, None, gen.seed, 0, 0, None, img),
                         "explicit_tensor": lambda: fs2.run(h2, x_T, zs, None, img)}, a.reps)
    assert torch.isfinite(img).all()
    return {"batch": B, "steps": N,
            "device_noise": dict(stats(times["device_noise"]), noise_bytes=4 * int(np.prod(shape))),      # one row, over all lanes
            "explicit_tensor": dict(stats(times["explicit_tensor"]), noise_bytes=int(explicit_bytes)),
            "ratio": float(np.median(times["device_noise"]) / np.median(times["explicit_tensor"]))}


def bench_guided(a):
    from rangeldm_amd import _lib, rng
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
    from rangeldm_amd.pipelines import LDMPipelineRange, _FusedSampler
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, repaint_program
    from rangeldm_amd.synth import normal, synth_state_dict
    from rangeldm_amd.unet import UNet2DModelHIP
    from rangeldm_amd.vae import AutoencoderKLHIP
    p = PRESETS["RangeLDM"]
    unet = UNet2DModelHIP(p["unet"])
    unet.load_state_dict(synth_state_dict(unet_param_shapes(p["unet"]), prefix=""))
    vae = AutoencoderKLHIP(p["vae"])
    vae.load_state_dict(synth_state_dict(vae_param_shapes(p["vae"]), prefix="vae."))
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=p["pos_encoding"])
    B = a.batch
    lat = (B, p["unet"].out_channels, *p["unet"].sample_size)
    f = p["vae"].downscale
    z0 = torch.from_numpy(normal(1, "bench/z0", lat)).cuda()
    mask = torch.ones((B, 1, *lat[2:]), device="cuda")
    mask[:, :, :lat[2] // 16] = 0
    img = torch.empty((B, p["vae"].out_channels, lat[2] * f, lat[3] * f), device="cuda")
    program = repaint_program(pipe.scheduler, 50, 10, 10)
    rows = len(program[0])
    fs = pipe._fused
    h = fs.get(unet, vae, pipe.scheduler, B, rows, _lib.RLDM_SAMPLER_DDIM, p["pos_encoding"], 0, program=program)
    gen = rng.DeviceGenerator(3)
    x_T = rng.randn(lat, gen.at(0))
    base = torch.cuda.memory_allocated()
    nk, nr = rng.randn_rows(rows, lat, gen, 0, 2), rng.randn_rows(rows, lat, gen, 0, 3)
    explicit_bytes = torch.cuda.memory_allocated() - base
    fs2 = _FusedSampler()                                            # (one sampler per variant: see bench_ddpm)
    h2 = fs2.get(unet, vae, pipe.scheduler, B, rows, _lib.RLDM_SAMPLER_DDIM, p["pos_encoding"], 0, program=program)
    times = interleaved({"device_noise": lambda: fs.run_guided_rng(h, x_T, gen.seed, 0, 0, z0, mask, img),
                         "explicit_tensors": lambda: fs2.run_guided(h2, x_T, None, z0, mask, nk, nr, img)}, a.reps)
    assert torch.isfinite(img).all()
    row_bytes = 4 * int(np.prod(lat))
    return {"batch": B, "rows": rows,
            "device_noise": dict(stats(times["device_noise"]), noise_bytes=2 * row_bytes),
            "explicit_tensors": dict(stats(times["explicit_tensors"]), noise_bytes=int(explicit_bytes)),
            "ratio": float(np.median(times["device_noise"]) / np.median(times["explicit_tensors"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="fill,ddpm,guided")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ddpm-steps", type=int, default=1000)
    ap.add_argument("--fill-iters", type=int, default=50)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    for name, fn in (("fill", bench_fill), ("ddpm", bench_ddpm), ("guided", bench_guided)):
        if name in a.only.split(","):
            out[name] = fn(a)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
