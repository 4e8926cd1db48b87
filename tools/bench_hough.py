#!/usr/bin/env python3
"""Time the Hough estimate of a sensor's tables (rangeldm_amd/csrc/hough.hip, rangeldm_amd/sensor.py) on a dataset-sized
input, next to the numpy statement on the host.

    python tools/bench_hough.py [--sweeps 256] [--width 2048] [--reps 5] [--workers 16] [--host-sweeps 16]

--sweeps synthetic sweeps of the KITTI-360 sensor (64 beams x --width azimuths, a fifth of the returns dropped: about 10^5
returns each), resident on the device, on HoughGrid.default().  Three legs, each the median [min, max] of --reps calls after one
warm-up call, each call synchronised:

    add            HoughAccumulator.add of all sweeps (pack + vote) into a cleared accumulator
    row_peaks      HoughAccumulator.row_peaks
    refine_beams   sensor.refine_beams of all sweeps against the picked beams (pack + assign + moments + the host's line fit)

and hough_votes_host on --host-sweeps of the sweeps shared out over --workers host processes, extrapolated linearly to --sweeps.
The device votes of those sweeps are checked against the host's (equal), and the recovered tables against the truth.

Vote rates: `considered` counts (valid return, row) pairs per second -- the arithmetic; `cast` counts the votes that landed in
a bin -- the LDS atomics.  `lds_atomic_assumed` is the rate the kernel's design took for granted: an LDS integer atomic issuing
like ds_write_b32, 64 lanes in two LDS cycles when no two lanes share a counter, on every CU at 2.4 GHz.  The host
leg runs first, in processes forked before the GPU is opened.
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

CLOCK_HZ = 2.4e9        # the MI355X's peak engine clock, which the assumed LDS-atomic rate is stated at
_HOST = None            # (sweeps, grid) of the host leg: set before the pool forks, read by its workers


def sweep(incl, height, W, seed):
    """(n, 3) fp32: per pixel a range exp(uniform(log 2.5, log 80)), the column's azimuth +- 0.4 of a column, a fifth dropped."""
    rng = np.random.default_rng(seed)
    H = len(incl)
    r = np.exp(rng.uniform(np.log(2.5), np.log(80.0), (W, H)))
    azi = ((W - 0.5 - np.arange(W)) / W * 2.0 * np.pi - np.pi)[:, None] + rng.uniform(-0.4, 0.4, (W, H)) * (2.0 * np.pi / W)
    xy, z = r * np.cos(incl)[None, :], height[None, :] - r * np.sin(incl)[None, :]
    return np.stack([xy * np.cos(azi), xy * np.sin(azi), z], -1)[rng.uniform(size=(W, H)) >= 0.2].astype(np.float32)


def _host_one(i):
    from rangeldm_amd.sensor import hough_votes_host
    sweeps, grid = _HOST
    return hough_votes_host([sweeps[i]], grid)


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


def time_host(sweeps, grid, reps, workers):
    global _HOST
    import rangeldm_amd.sensor  # noqa: F401  (imported before the fork: no worker pays for it inside a timed call)
    _HOST = (sweeps, grid)
    with mp.get_context("fork").Pool(workers) as pool:
        ts, parts = time_calls(lambda: pool.map(_host_one, range(len(sweeps))), reps)
    return ts, sum(p.astype(np.uint64) for p in parts).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=256)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-sweeps", type=int, default=16)
    a = ap.parse_args()
    from rangeldm_amd.range_image import _KITTI_HEIGHT, _KITTI_ZENITH
    from rangeldm_amd import sensor as S
    incl, height = -np.array(_KITTI_ZENITH, np.float64), np.array(_KITTI_HEIGHT, np.float64)
    grid = S.HoughGrid.default()
    sweeps = [sweep(incl, height, a.width, s) for s in range(a.sweeps)]
    n_host = min(a.host_sweeps, a.sweeps)
    th, host_votes = time_host(sweeps[:n_host], grid, a.reps, a.workers)                 # before the GPU is opened: the pool forks

    import torch
    dev = torch.device("cuda")
    clouds = [torch.from_numpy(c).to(dev) for c in sweeps]
    acc = S.HoughAccumulator(grid, dev)

    def run_add():
        acc.votes().zero_()
        acc.points = 0
        acc.add(clouds)
        torch.cuda.synchronize()
        return acc.points

    def run_peaks():
        mx, arg = acc.row_peaks()
        torch.cuda.synchronize()
        return mx.cpu().numpy(), arg.cpu().numpy()

    ta, points = time_calls(run_add, a.reps)
    tp, peaks = time_calls(run_peaks, a.reps)
    cast = int(acc.votes().cpu().numpy().astype(np.uint64).sum())
    h_incl, h_height, _ = S.pick_beams(peaks[0], peaks[1], 64, 4, grid)

    def run_refine():
        out = S.refine_beams(clouds, h_incl, h_height, 2.0 * grid.theta_step, d_min=grid.d_min, d_max=grid.d_max, device=dev)
        torch.cuda.synchronize()
        return out

    tr, fine = time_calls(run_refine, a.reps)
    check = S.HoughAccumulator(grid, dev).add(clouds[:n_host])
    if not np.array_equal(check.votes().cpu().numpy(), host_votes):
        raise SystemExit("the device votes differ from hough_votes_host")
    add, host = spread(ta), spread(th)
    host_all = host["seconds"] * a.sweeps / n_host
    props = torch.cuda.get_device_properties(0)
    assumed = 32.0 * props.multi_processor_count * CLOCK_HZ                          # lane-adds per second
    out = {"device": torch.cuda.get_device_name(0), "sweeps": a.sweeps, "points": points, "grid": [grid.n_theta, grid.n_h],
           "rows_per_workgroup": S.vote_shape(points, grid)[0], "add": add, "row_peaks": spread(tp), "refine_beams": spread(tr),
           "hough_votes_host": {**host, "sweeps": n_host, "workers": a.workers, "seconds_extrapolated": host_all},
           "host_over_add": host_all / add["seconds"],
           "votes_considered_per_s": points * grid.n_theta / add["seconds"], "votes_cast": cast,
           "votes_cast_per_s": cast / add["seconds"], "lds_atomic_assumed_per_s": assumed,
           "cast_over_assumed": cast / add["seconds"] / assumed,
           "worst_incl_error_rad": float(np.abs(fine[0] - incl).max()), "worst_height_error_m": float(np.abs(fine[1] - height).max()),
           "equals_host": True}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
