#!/usr/bin/env python3
"""Time farthest point sampling (rangeldm_amd/csrc/fps.hip, metrics.farthest_point_sample) on synthetic LiDAR-like sweeps:
256 clouds of 65 536 points (the resident tier: a generated range image), k = 2 048, repeated five times after one warm-up
call and reported as median [min, max]; one cloud of 131 072 points (the workspace tier) the same way; and, in the same
session, the host route it replaces: the numpy restatement of tests/test_fps_host.py (fps_host) in 16 worker processes over a
few of the same clouds, EXTRAPOLATED to the whole batch and labelled so.  The device indices of those clouds must equal the
host's.

    python tools/bench_fps.py [--clouds 256] [--points 65536] [--k 2048] [--reps 5] [--host-clouds 16] [--big-points 131072]

Time is a host clock around rldm_farthest_point_sample on a pre-packed batch; the call synchronises the stream before it
returns.  The host baseline runs first, before this process opens the GPU (its workers are forked).  A round is one update of
the min-distance array plus the arg-max; "distance evaluations" are rounds x points (k - 1 rounds per cloud: the last index
needs no update).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def _host_one(job):
    from test_fps_host import fps_host
    cloud, k = job
    t0 = time.perf_counter()
    idx = fps_host(cloud, k, 0)
    return time.perf_counter() - t0, idx


def host_baseline(clouds, k, workers):
    """Wall seconds per cloud with `workers` processes busy, and each cloud's indices."""
    import multiprocessing as mp
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_host_one, [(c[:256], 8) for c in clouds[:workers]])     # start the workers
        t0 = time.perf_counter()
        res = pool.map(_host_one, [(c, k) for c in clouds], chunksize=1)
        wall = time.perf_counter() - t0
    return {"clouds": len(clouds), "workers": workers, "wall_seconds_per_cloud": wall / len(clouds),
            "one_worker_seconds_per_cloud_median": float(np.median([r[0] for r in res]))}, [r[1] for r in res]


def time_case(clouds, k, reps, label):
    import torch
    from rangeldm_amd import _lib
    from rangeldm_amd.metrics import _pack
    xp, xo, xk = _pack(clouds)
    idx = torch.empty((len(clouds), k), dtype=torch.int32, device=xp.device)
    L, st = _lib.lib(), _lib.stream_ptr(xp.device)

    def run():
        _lib.check(L.rldm_farthest_point_sample(xp.data_ptr(), xo.data_ptr(), xk, len(clouds), k, None, idx.data_ptr(), st),
                   "rldm_farthest_point_sample")
        torch.cuda.synchronize()
    run()                                                # warm-up: code object load, allocator
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
        print(f"  {label}: repetition {len(ts)} took {ts[-1] * 1e3:.2f} ms", file=sys.stderr, flush=True)
    return ts, idx


def summary(label, ts, clouds, points, k):
    med = float(np.median(ts))
    rounds = clouds * (k - 1)
    return {"case": label, "clouds": clouds, "points": points, "k": k, "reps": len(ts), "seconds": med, "seconds_min": min(ts),
            "seconds_max": max(ts), "ms_per_cloud": 1e3 * med / clouds, "rounds_per_s": rounds / med,
            "distance_evaluations_per_s": rounds * points / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--k", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-clouds", type=int, default=16, help="clouds the host baseline samples (extrapolated to --clouds)")
    ap.add_argument("--host-workers", type=int, default=16)
    ap.add_argument("--big-points", type=int, default=131072, help="size of the single cloud that shows the workspace tier")
    a = ap.parse_args()
    from test_fps_host import lidar_like
    rng = np.random.default_rng(1)
    clouds_h = [lidar_like(rng, a.points) for _ in range(a.clouds)]
    big_h = lidar_like(rng, a.big_points)
    # the host route first: its workers are forked, so the GPU must not be open yet
    hc = min(a.host_clouds, a.clouds)
    host, host_idx = host_baseline(clouds_h[:hc], a.k, a.host_workers)
    host["extrapolated_seconds_for_all_clouds"] = host["wall_seconds_per_cloud"] * a.clouds
    host["note"] = f"measured on {hc} clouds, extrapolated linearly to {a.clouds}"

    import torch
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "host_fps_host_numpy": host, "runs": []}
    ts, idx = time_case([torch.from_numpy(c).to(dev) for c in clouds_h], a.k, a.reps, "resident tier")
    run = summary(f"{a.clouds} clouds of {a.points} points, k = {a.k}", ts, a.clouds, a.points, a.k)
    run["equals_host_on_the_host_clouds"] = bool(np.array_equal(idx[:hc].cpu().numpy(), np.stack(host_idx)))
    run["speedup_vs_host_16_workers_extrapolated"] = host["extrapolated_seconds_for_all_clouds"] / run["seconds"]
    out["runs"].append(run)
    ts, _ = time_case([torch.from_numpy(big_h).to(dev)], a.k, a.reps, "workspace tier")
    out["runs"].append(summary(f"1 cloud of {a.big_points} points, k = {a.k}", ts, 1, a.big_points, a.k))
    ts, _ = time_case([torch.from_numpy(clouds_h[0]).to(dev)], a.k, a.reps, "one resident cloud")
    out["runs"].append(summary(f"1 cloud of {a.points} points, k = {a.k}", ts, 1, a.points, a.k))
    print(json.dumps(out, indent=1))
    if not run["equals_host_on_the_host_clouds"]:
        raise SystemExit("the device indices differ from fps_host")


if __name__ == "__main__":
    main()
