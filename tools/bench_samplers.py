#!/usr/bin/env python3
"""Images per second of the captured LDMPipelineRange call for each shipped sampler at the same batch, box and weights (synthetic):
DDPM-50 (the RangeLDM config as shipped), DDIM-50 (the bench.py headline), DPM-Solver++(2M) at 20 and 25 steps, UniPC at 10 and 15.
`--only NAME-STEPS[,NAME-STEPS...]` measures those samplers alone (any of the schedulers at any step count), in the order given.  One pipeline call =
x_T -> every step -> VAE decode; HIP events around `--iters` calls after `--warmup` (the first builds the sampler and captures its
graphs), `--rounds` times with the samplers taking turns: the median [min, max] of the rounds.  Prints one JSON line.

    python tools/bench_samplers.py [--B 16] [--preset RangeLDM] [--iters 20] [--warmup 3] [--rounds 1] [--only unipc-10,dpmsolver++-10]

Speed only: how closely 20 DPM++ steps match 50 DDIM / DDPM steps on trained weights is not measured here
(tests/test_dpmsolver_host.py and tests/test_unipc_host.py check the solvers' accuracy on data whose exact solution is known)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

SAMPLERS = (("ddpm", 50), ("ddim", 50), ("dpmsolver++", 20), ("dpmsolver++", 25), ("unipc", 10), ("unipc", 15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--preset", default="RangeLDM")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1, help="alternating rounds of --iters calls per sampler: median [min, max] over them")
    ap.add_argument("--only", default=None, help="comma-separated NAME-STEPS list, e.g. unipc-10,dpmsolver++-10")
    a = ap.parse_args()
    samplers = SAMPLERS if a.only is None else tuple((s.rsplit("-", 1)[0], int(s.rsplit("-", 1)[1])) for s in a.only.split(","))
    from rangeldm_amd.inference import make_scheduler
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.synth import latent_noise
    p, unet, vae, _, _ = bench.build_models(a.preset, 0)
    if vae is None:
        raise SystemExit(f"{a.preset}: a latent-space preset is needed (LDMPipelineRange)")
    dev = torch.device("cuda")
    shape = (p["unet"].out_channels, *p["unet"].sample_size)
    x_T = torch.from_numpy(np.stack([latent_noise(1, j, shape) for j in range(a.B)])).to(dev)
    runs = []
    for name, steps in samplers:
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_scheduler(name, None), pos_encoding=p["pos_encoding"])
        kw = dict(batch_size=a.B, num_inference_steps=steps, latents=x_T, output_type="torch")
        if name == "ddpm":                              # the ancestral noise resident on the device, as bench.py's inputs are
            kw["step_noise"] = torch.randn((steps, *x_T.shape), device=dev, generator=torch.Generator(dev).manual_seed(2))
        for _ in range(a.warmup):
            pipe(**kw)
        runs.append((f"{name}-{steps}", pipe, kw, []))
    torch.cuda.synchronize()
    for _ in range(a.rounds):                           # alternating: every sampler once per round, so a drift of the box hits all alike
        for key, pipe, kw, ms in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                pipe(check=False, **kw)
            e1.record()
            torch.cuda.synchronize()
            pipe._fused.status_all()                    # raises if a call of the loop tripped the persistent launches' self-check
            ms.append(e0.elapsed_time(e1) / a.iters)
    res = {}
    for key, _, _, ms in runs:
        med = float(np.median(ms))
        res[key] = {"ms_per_batch": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                    "img_per_s": round(a.B * 1000.0 / med, 1)}
        print(f"{key:>15}: {med:8.3f} ms [{min(ms):.3f}, {max(ms):.3f}] / batch of {a.B}  {a.B * 1000.0 / med:7.1f} img/s", file=sys.stderr)
    print(json.dumps({"tool": "bench_samplers", "preset": a.preset, "batch": a.B, "iters": a.iters, "rounds": a.rounds, "samplers": res,
                      "quality": "not measured: synthetic weights"}))


if __name__ == "__main__":
    main()
