#!/usr/bin/env python3
"""What decoder guidance (rangeldm_amd/guidance.py: DDIM whose clean estimate is guided through the VAE decoder's input gradient)
costs on the headline workload: RangeLDM, 50-step DDIM (eta = 0) + VAE decode, batch 16, KITTI-360 shapes, synthetic weights, every 4th
beam known -- in ONE process on one GPU, interleaved round by round so that clock and temperature drift hits all of them alike:

  (a) unguided_fused     the headline sampler (the captured loop)
  (b) unguided_eager     fused=False: the Python loop the guided call extends, one unet / scheduler call per step
  (c) decoder_guided     LDMPipelineRange(decoder_guidance=..., guidance_iters = --iters): (b) + per step a tape decode, the residual,
                         the input-gradient-only replay, the update and the correction
  (d) rangedm_guided     the pixel-space route to densification: RangeDM, known-region replacement, the same mask, 50 rows
  (e) rangedm_repaint    the same with RePaint's defaults (jump_length = 10, jump_n_sample = 10: 410 rows)

    python tools/bench_decoder_guidance.py [--reps 5] [--batch 16] [--steps 50] [--iters 1] [--no-rangedm]

One warm-up call of each, then --reps rounds of one timed call each (host clock around the call and a device synchronise): median
[min, max] seconds per call.  Then one instrumented guided call: every library call of a guided step between two device events (a
call is one launch, except `unet`, which is the UNet's whole eager launch sequence, and the deterministic-mode folds), summed per
part -- UNet, scheduler, decoder forward, input-gradient replay, the kernels of csrc/guide.hip -- as the per-step split, and the three
most expensive single calls of a step.  Event timing serialises the calls, so the split adds up to more than (c)'s time per step.  A
kernel trace (`rocprofv3 --kernel-trace --stats -- python tools/bench_decoder_guidance.py --reps 1 --no-rangedm`) belongs in a run
of its own.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def instrument(pipe, guide, call, steps):
    """One guided call with every train_ops / unet / scheduler call between device events -> (ms per part and step, top three calls)."""
    from rangeldm_amd import train_ops as T
    records, phase = [], ["other"]

    def timed(name, fn, part=None):
        def wrapper(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            shape = tuple(a[0].shape) if a and torch.is_tensor(a[0]) else ()
            records.append((part or phase[0], name, shape, e0, e1))
            return out
        return wrapper

    saved = {}
    for name in ("conv", "conv_fused", "gn_forward", "gn_backward", "add", "sum2x2", "silu", "silu_backward"):
        saved[name] = getattr(T, name)
        setattr(T, name, timed(name, saved[name]))
    for name in ("guide_residual", "guide_latent", "guide_update", "guide_correct"):
        saved[name] = getattr(T, name)
        setattr(T, name, timed(name, saved[name], "guide_kernels"))
    fwd, bwd = guide.forward, guide.input_gradient

    def forward(*a, **k):
        phase[0] = "decoder_forward"
        try:
            return fwd(*a, **k)
        finally:
            phase[0] = "other"

    def input_gradient(*a, **k):
        phase[0] = "input_gradient_replay"
        try:
            return bwd(*a, **k)
        finally:
            phase[0] = "other"
    guide.forward, guide.input_gradient = forward, input_gradient
    unet_call, launch = type(pipe.unet).__call__, pipe.scheduler._launch
    type(pipe.unet).__call__ = timed("unet", unet_call, "unet")
    pipe.scheduler._launch = timed("sched_step", launch, "scheduler")
    try:
        call()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(T, name, fn)
        del guide.forward, guide.input_gradient
        type(pipe.unet).__call__ = unet_call
        del pipe.scheduler._launch
    parts, calls = {}, {}
    for part, name, shape, e0, e1 in records:
        ms = e0.elapsed_time(e1)
        parts[part] = parts.get(part, 0.0) + ms
        key = (part, name, shape)
        n, tot = calls.get(key, (0, 0.0))
        calls[key] = (n + 1, tot + ms)
    split = {k: v / steps for k, v in sorted(parts.items())}
    split["calls_per_step"] = len(records) / steps
    single = [c for c in calls.items() if c[0][1] != "unet"]
    top = sorted(single, key=lambda c: -c[1][1] / c[1][0])[:3]
    return split, [{"part": k[0], "call": k[1], "first_operand": list(k[2]), "ms_per_call": tot / n, "calls_per_step": n / steps}
                   for k, (n, tot) in top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-rangedm", action="store_true", help="skip the pixel-space samplers (d), (e)")
    a = ap.parse_args()

    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.guidance import DecoderGuide
    from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
    from rangeldm_amd.pipelines import DDIMPipelineRange, LDMPipelineRange
    from rangeldm_amd.schedulers import DDIMSchedulerHIP
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
    guide = DecoderGuide(vae)
    B, N = a.batch, a.steps
    lat = (B, p["unet"].out_channels, *p["unet"].sample_size)
    f = p["vae"].downscale
    W, H = lat[2] * f, lat[3] * f
    x_T = torch.from_numpy(normal(1, "bench/xT", lat)).to(dev)
    known = (torch.from_numpy(normal(1, "bench/known", (B, 2, W, H))) * 0.5).to(dev)
    mask = torch.zeros((B, 1, W, H), device=dev)
    mask[..., 2::4] = 1                                            # every 4th beam
    common = dict(batch_size=B, num_inference_steps=N, latents=x_T, output_type="torch")
    guided_kw = dict(common, known=known, known_mask=mask, decoder_guidance=guide, guidance_scale=a.scale, guidance_iters=a.iters)
    cases = {"unguided_fused": (N, lambda: pipe(**common)),
             "unguided_eager": (N, lambda: pipe(fused=False, **common)),
             "decoder_guided": (N, lambda: pipe(**guided_kw))}
    if not a.no_rangedm:
        from rangeldm_amd.schedulers import repaint_program
        q = PRESETS["RangeDM"]
        px = UNet2DModelHIP(q["unet"])
        px.load_state_dict(synth_state_dict(unet_param_shapes(q["unet"]), prefix="dm."))
        dm = DDIMPipelineRange(unet=px, scheduler=DDIMSchedulerHIP(), pos_encoding=q["pos_encoding"])
        shape = (B, q["unet"].out_channels, *q["unet"].sample_size)
        if tuple(shape[2:]) != (W, H):
            raise RuntimeError(f"RangeDM samples {shape[2:]}, RangeLDM's images are {(W, H)}")
        xp = torch.from_numpy(normal(1, "bench/xT_dm", shape)).to(dev)
        for name, jl, jn in (("rangedm_guided", 1, 1), ("rangedm_repaint", 10, 10)):
            rows = len(repaint_program(dm.scheduler, N, jl, jn)[0])
            nk = torch.randn((rows, *shape), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
            nr = torch.randn((rows, *shape), generator=torch.Generator(device=dev).manual_seed(3), device=dev) if jn > 1 else None
            kw = dict(batch_size=B, num_inference_steps=N, latents=xp, known=known, known_mask=mask, jump_length=jl, jump_n_sample=jn,
                      known_noise=nk, renoise_noise=nr, output_type="torch")
            cases[name] = (rows, lambda kw=kw: dm(**kw))
    times = {k: [] for k in cases}
    for k, (_, run) in cases.items():                               # warm-up: plans, graph capture, scratch buffers
        out = run()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), k
    for _ in range(a.reps):
        for k, (_, run) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "steps": N, "guidance_iters": a.iters, "reps": a.reps, "samplers": {}}
    for k, (rows, _) in cases.items():
        ts = times[k]
        med = float(np.median(ts))
        res["samplers"][k] = {"rows": rows, "seconds": med, "seconds_min": min(ts), "seconds_max": max(ts), "ms_per_row": 1e3 * med / rows,
                              "images_per_s": B / med}
    s = res["samplers"]
    res["guided_vs_eager"] = s["decoder_guided"]["seconds"] / s["unguided_eager"]["seconds"]
    res["guided_vs_fused"] = s["decoder_guided"]["seconds"] / s["unguided_fused"]["seconds"]
    res["guidance_ms_per_step"] = 1e3 * (s["decoder_guided"]["seconds"] - s["unguided_eager"]["seconds"]) / N
    if "rangedm_guided" in s:
        res["guided_vs_rangedm_guided"] = s["decoder_guided"]["seconds"] / s["rangedm_guided"]["seconds"]
    res["step_split_ms"], res["top_calls"] = instrument(pipe, guide, lambda: pipe(**guided_kw), N)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
