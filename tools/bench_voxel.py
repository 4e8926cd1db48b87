#!/usr/bin/env python3
"""Time the voxel-occupancy kernel (rangeldm_amd/csrc/voxel.hip) on KITTI-size pairs at voxel = 0.1 m, next to what the same
command already pays for the Chamfer distance and to the numpy statement on the host.

    python tools/bench_voxel.py [--pairs 8 1000] [--points 60000] [--voxel 0.1] [--reps 5] [--workers 16]

Per pair count, three legs, each the median [min, max] of --reps calls after one warm-up call:

    voxel_counts       metrics.voxel_counts on the device clouds (packing and the call's own synchronisation included)
    chamfer_pairs      metrics.chamfer_pairs on the same pairs
    voxel_counts_host  metrics.voxel_counts_host, the pairs shared out over --workers host processes

and the two ratios the feature is judged by: voxel_counts / chamfer_pairs (what --voxel adds to a command that already pays for
the CD) and voxel_counts_host / voxel_counts.  Clouds come from bench_chamfer.py's generator (54-66 k points, 3-70 m); the
target of a pair is its result cloud with a fifth of the points dropped and the rest jittered by 3 cm, so the two occupancy
sets overlap in part, as a reconstruction's do.  The host leg runs first, in processes forked before the GPU is opened.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

_PAIRS = None           # (xs, ys, voxel) of the host leg: set before the pool forks, read by its workers


def kitti_like(rng, n):
    r = rng.uniform(3.0, 70.0, n)
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.43, 0.03, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el) + 1.7], 1).astype(np.float32)


def make_pairs(pairs, points, seed=1):
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    for n in rng.integers(points - points // 10, points + points // 10 + 1, pairs).tolist():
        x = kitti_like(rng, n)
        keep = rng.random(n) < 0.8
        xs.append(x)
        ys.append((x[keep] + 0.03 * rng.standard_normal((int(keep.sum()), 3))).astype(np.float32))
    return xs, ys


def _host_slice(bounds):
    from rangeldm_amd.metrics import voxel_counts_host
    xs, ys, voxel = _PAIRS
    lo, hi = bounds
    return voxel_counts_host(xs[lo:hi], ys[lo:hi], voxel)


def spread(ts):
    return {"seconds": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "reps": len(ts)}


def time_calls(fn, reps):
    out = fn()                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def time_host(xs, ys, voxel, reps, workers):
    global _PAIRS
    import rangeldm_amd.metrics  # noqa: F401  (imported before the fork: no worker pays for it inside a timed call)
    _PAIRS = (xs, ys, voxel)
    step = max(1, -(-len(xs) // (4 * workers)))          # four slices per worker: the tail of an uneven share stays short
    bounds = [(lo, min(len(xs), lo + step)) for lo in range(0, len(xs), step)]
    with mp.get_context("fork").Pool(workers) as pool:
        ts, parts = time_calls(lambda: pool.map(_host_slice, bounds), reps)
    return ts, np.concatenate(parts, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 1000])
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    sets = {n: make_pairs(n, a.points) for n in a.pairs}
    host = {n: time_host(*sets[n], a.voxel, a.reps, a.workers) for n in a.pairs}     # before the GPU is opened: the pool forks

    import torch
    from rangeldm_amd.metrics import chamfer_pairs, voxel_counts
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "voxel": a.voxel, "host_workers": a.workers, "runs": []}
    for n in a.pairs:
        xs = [torch.from_numpy(c).to(dev) for c in sets[n][0]]
        ys = [torch.from_numpy(c).to(dev) for c in sets[n][1]]

        def run_voxel():
            counts = voxel_counts(xs, ys, a.voxel)
            torch.cuda.synchronize()
            return counts

        def run_chamfer():
            xm, ym = chamfer_pairs(xs, ys)
            torch.cuda.synchronize()
            return xm + ym

        tv, counts = time_calls(run_voxel, a.reps)
        tc, cd = time_calls(run_chamfer, a.reps)
        th, want = host[n]
        if counts.cpu().numpy().tolist() != want.tolist():
            raise SystemExit(f"{n} pairs: the device counts differ from voxel_counts_host")
        f = counts.double()
        v, c, h = spread(tv), spread(tc), spread(th)
        out["runs"].append({"pairs": n, "points_per_pair": (sum(len(c_) for c_ in sets[n][0]) + sum(len(c_) for c_ in sets[n][1])) / n,
                            "voxel_counts": v, "chamfer_pairs": c, "voxel_counts_host": h,
                            "voxel_over_chamfer": v["seconds"] / c["seconds"], "host_over_voxel": h["seconds"] / v["seconds"],
                            "mean_iou": float((f[:, 2] / (f[:, 0] + f[:, 1] - f[:, 2])).mean()), "mean_cd": float(cd.mean()),
                            "equals_host": True})
        del xs, ys
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
