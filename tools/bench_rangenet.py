#!/usr/bin/env python3
"""Time RangeNet++ inference (rangeldm_amd/csrc/rangenet.hip, rangenet.RangeNet.infer) on synthetic DarkNet53 weights at
64 x 1024: scans per second at batch 1 and batch 8, each the median [min, max] of five repetitions after one warm-up call (a
repetition is `--iters` forwards between two stream synchronisations).  In the same run, on the same GPU: the torch route it
stands beside, rangenet.forward_host(bf16=True, device="cuda") -- the same arithmetic through torch's conv (MIOpen), fp32
tensors holding bf16 values -- and rldm_calibrate's pure-MFMA rate, against which the forward's FLOP/s
(rangenet.network_flops: the taps that reach an output) are reported as a fraction.

    python tools/bench_rangenet.py [--layers 53] [--batches 1 8] [--reps 5] [--iters 10] [--torch-iters 2]

Read the figures as medians with their spread; a single repetition on a shared machine says little.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def timed(fn, reps, iters, label):
    import torch
    fn()                                                 # warm-up: code object load, arena, MIOpen's search
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters)
        print(f"  {label}: repetition {len(ts)}: {ts[-1] * 1e3:.2f} ms per forward", file=sys.stderr, flush=True)
    return ts


def summary(ts, batch, flops, mfma_tflops):
    med = float(np.median(ts))
    return {"seconds": med, "seconds_min": min(ts), "seconds_max": max(ts), "scans_per_s": batch / med,
            "scans_per_s_min": batch / max(ts), "scans_per_s_max": batch / min(ts), "tflops": batch * flops / med / 1e12,
            "fraction_of_mfma_rate": batch * flops / med / 1e12 / mfma_tflops}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=53, choices=(21, 53))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    a = ap.parse_args()
    import torch
    from rangeldm_amd import _lib
    from rangeldm_amd import rangenet as R
    dev = torch.device("cuda")
    arch = R.synthetic_arch(a.layers)
    state = R.fold_state(arch, *R.synthetic_state(arch))
    net = R.RangeNet(state)
    state_dev = R.state_to(state, dev)
    H, W = 64, 1024
    flops = R.network_flops(state, H, W)
    cal = [C.c_double(), C.c_double(), C.c_double()]
    _lib.check(_lib.lib().rldm_calibrate(C.byref(cal[0]), C.byref(cal[1]), C.byref(cal[2]), _lib.stream_ptr(dev)), "rldm_calibrate")
    out = {"device": torch.cuda.get_device_name(0), "layers": a.layers, "shape": [H, W], "gflop_per_scan": flops / 1e9,
           "calibration": {"mfma_tflops": cal[0].value, "mfma_clock_mhz": cal[1].value, "copy_gbs": cal[2].value}, "runs": []}
    proj, _ = R.project_scan(*R.synthetic_cloud(1))
    for batch in a.batches:
        x = torch.from_numpy(proj)[None].repeat(batch, 1, 1, 1).to(dev)
        ours = timed(lambda: net.infer(x), a.reps, a.iters, f"batch {batch}, librangeldm_hip")
        with torch.no_grad():
            theirs = timed(lambda: R.forward_host(state_dev, x, bf16=True, device=dev), a.reps, a.torch_iters, f"batch {batch}, torch")
        run = {"batch": batch, "librangeldm_hip": summary(ours, batch, flops, cal[0].value),
               "torch_forward_host_bf16": summary(theirs, batch, flops, cal[0].value)}
        run["speedup_vs_torch"] = run["torch_forward_host_bf16"]["seconds"] / run["librangeldm_hip"]["seconds"]
        out["runs"].append(run)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
