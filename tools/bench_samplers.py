#!/usr/bin/env python3
"""Images per second of the captured LDMPipelineRange call for each shipped sampler at the same batch, box and weights (synthetic):
DDPM-50 (the RangeLDM config as shipped), DDIM-50 (the bench.py headline), DPM-Solver++(2M) at 20 and 25 steps.  One pipeline call =
x_T -> every step -> VAE decode; HIP events around `--iters` calls after `--warmup` (the first builds the sampler and captures its
graphs).  Prints one JSON line.

    python tools/bench_samplers.py [--B 16] [--preset RangeLDM] [--iters 20] [--warmup 3]

Speed only: how closely 20 DPM++ steps match 50 DDIM / DDPM steps on trained weights is not measured here
(tests/test_dpmsolver_host.py checks the solver's accuracy on data whose exact solution is known)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

SAMPLERS = (("ddpm", 50), ("ddim", 50), ("dpmsolver++", 20), ("dpmsolver++", 25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--preset", default="RangeLDM")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from rangeldm_amd.inference import make_scheduler
    from rangeldm_amd.pipelines import LDMPipelineRange
    from rangeldm_amd.synth import latent_noise
    p, unet, vae, _, _ = bench.build_models(a.preset, 0)
    if vae is None:
        raise SystemExit(f"{a.preset}: a latent-space preset is needed (LDMPipelineRange)")
    dev = torch.device("cuda")
    shape = (p["unet"].out_channels, *p["unet"].sample_size)
    x_T = torch.from_numpy(np.stack([latent_noise(1, j, shape) for j in range(a.B)])).to(dev)
    res = {}
    for name, steps in SAMPLERS:
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_scheduler(name, None), pos_encoding=p["pos_encoding"])
        kw = dict(batch_size=a.B, num_inference_steps=steps, latents=x_T, output_type="torch")
        if name == "ddpm":                              # the ancestral noise resident on the device, as bench.py's inputs are
            kw["step_noise"] = torch.randn((steps, *x_T.shape), device=dev, generator=torch.Generator(dev).manual_seed(2))
        for _ in range(a.warmup):
            pipe(**kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            pipe(check=False, **kw)
        e1.record()
        torch.cuda.synchronize()
        pipe._fused.status_all()                        # raises if a call of the loop tripped the persistent launches' self-check
        ms = e0.elapsed_time(e1) / a.iters
        res[f"{name}-{steps}"] = {"ms_per_batch": round(ms, 3), "img_per_s": round(a.B * 1000.0 / ms, 1)}
        print(f"{name:>12}-{steps}: {ms:8.3f} ms / batch of {a.B}  {a.B * 1000.0 / ms:7.1f} img/s", file=sys.stderr)
        del pipe
    print(json.dumps({"tool": "bench_samplers", "preset": a.preset, "batch": a.B, "iters": a.iters, "samplers": res,
                      "quality": "not measured: synthetic weights"}))


if __name__ == "__main__":
    main()
