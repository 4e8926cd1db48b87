#!/usr/bin/env python3
"""What guided sampling (known-region replacement on the unconditional weights, rldm_sample_guided) costs on the headline
workload: RangeLDM, 50-step DDIM (eta = 0) + VAE decode, batch 16 -- four samplers in ONE process on one GPU, interleaved
round by round so that clock and temperature drift hits all of them alike:

  (a) unguided           the headline sampler (scheduler step in conv_out's epilogue)
  (b) unguided_separate  the same with Flag.SCHED_LAUNCH: the scheduler step as a launch of its own -- the yardstick for (c)
  (c) guided             jump_n_sample = 1: the rows of (b), each reading known / mask / known_noise as well
  (d) guided_repaint     jump_length = 10, jump_n_sample = 10 (RePaint's defaults): 50 + 9 * 10 * 4 = 410 rows

    python tools/bench_guided.py [--reps 5] [--batch 16] [--steps 50]

One warm-up call of each (plans, graph capture), then --reps rounds of one timed call each (host clock around the call and a
device synchronise).  Reported per sampler: the median, min and max seconds per call, the rows and the time per row; then
(c) against (b) next to (b)'s own min-max spread, and (d)'s time per row against (c)'s.  Prints one JSON object.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--jump-length", type=int, default=10)
    ap.add_argument("--jump-n-sample", type=int, default=10)
    a = ap.parse_args()

    from rangeldm_amd import _lib
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP, repaint_program
    from rangeldm_amd.synth import normal, synth_state_dict
    from rangeldm_amd.unet import UNet2DModelHIP
    from rangeldm_amd.vae import AutoencoderKLHIP

    p = PRESETS["RangeLDM"]
    dev = torch.device("cuda")
    unet = UNet2DModelHIP(p["unet"])
    unet.load_state_dict(synth_state_dict(unet_param_shapes(p["unet"]), prefix=""))
    vae = AutoencoderKLHIP(p["vae"])
    vae.load_state_dict(synth_state_dict(vae_param_shapes(p["vae"]), prefix="vae."))
    pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=DDIMSchedulerHIP(), pos_encoding=p["pos_encoding"])
    B, N = a.batch, a.steps
    lat = (B, p["unet"].out_channels, *p["unet"].sample_size)
    f = p["vae"].downscale
    x_T = torch.from_numpy(normal(1, "bench/xT", lat)).to(dev)
    z0 = torch.from_numpy(normal(1, "bench/z0", lat)).to(dev)
    mask = torch.ones((B, 1, *lat[2:]), device=dev)
    mask[:, :, :lat[2] // 16] = 0                                   # the in-painting preset's span: 1/16 of the azimuth unknown
    img = torch.empty((B, p["vae"].out_channels, lat[2] * f, lat[3] * f), device=dev)
    fs = pipe._fused

    def unguided(flags):
        h = fs.get(unet, vae, pipe.scheduler, B, N, _lib.RLDM_SAMPLER_DDIM, p["pos_encoding"], 0, plan_flags=flags)
        return N, lambda: fs.run(h, x_T, None, None, img)

    def guided(jl, jn):
        program = repaint_program(pipe.scheduler, N, jl, jn)
        rows = len(program[0])
        g = torch.Generator(device=dev).manual_seed(2)
        nk = torch.randn((rows, *lat), generator=g, device=dev)
        nr = torch.randn((rows, *lat), generator=g, device=dev) if jn > 1 else None
        h = fs.get(unet, vae, pipe.scheduler, B, rows, _lib.RLDM_SAMPLER_DDIM, p["pos_encoding"], 0, program=program)
        return rows, lambda: fs.run_guided(h, x_T, None, z0, mask, nk, nr, img)

    cases = {"unguided": unguided(0), "unguided_separate": unguided(int(_lib.Flag.SCHED_LAUNCH)), "guided": guided(1, 1),
             "guided_repaint": guided(a.jump_length, a.jump_n_sample)}
    times = {k: [] for k in cases}
    for k, (_, run) in cases.items():                               # warm-up: plans, eager step, graph capture
        run()
        torch.cuda.synchronize()
        assert torch.isfinite(img).all(), k
    for _ in range(a.reps):
        for k, (_, run) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()                                                   # (run checks rldm_sampler_status: it waits for the call)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "steps": N, "reps": a.reps, "samplers": {}}
    for k, (rows, _) in cases.items():
        ts = times[k]
        med = float(np.median(ts))
        out["samplers"][k] = {"rows": rows, "seconds": med, "seconds_min": min(ts), "seconds_max": max(ts),
                              "ms_per_row": 1e3 * med / rows, "images_per_s": B / med}
    s = out["samplers"]
    b, c, d = s["unguided_separate"], s["guided"], s["guided_repaint"]
    out["guided_vs_separate"] = {"ratio": c["seconds"] / b["seconds"], "delta_ms": 1e3 * (c["seconds"] - b["seconds"]),
                                 "separate_spread_ms": 1e3 * (b["seconds_max"] - b["seconds_min"]),
                                 "within_spread": b["seconds_min"] <= c["seconds"] <= b["seconds_max"]}
    out["repaint_vs_guided_per_row"] = d["ms_per_row"] / c["ms_per_row"]
    out["separate_vs_fused_tail"] = b["seconds"] / s["unguided"]["seconds"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
