#!/usr/bin/env python3
"""Time the Earth Mover's Distance matrix (rangeldm_amd/csrc/emd.hip, metrics.emd_matrix) on synthetic LiDAR-like clouds:
64 x 64 and 1 000 x 1 000 clouds of 2 048 points, each case repeated five times after one warm-up call and reported as
median [min, max] with the mean number of bids per pair; and, in the same session, the host route it replaces:
scipy.optimize.linear_sum_assignment on the fp32 cost matrix, 16 worker processes, over a sample of the same pairs.

    python tools/bench_emd.py [--cases 64x64 1000x1000] [--points 2048] [--reps 5] [--host-pairs 32] [--eps 0.0078125]

Time is a host clock around emd_matrix-equivalent calls of rldm_emd_matrix on pre-packed sets; the call synchronises the
stream before it returns.  The host baseline runs first, before this process opens the GPU (its workers are forked).

Instruction count, read from the ISA of emd_auction_kernel<32>'s bidding loop (hipcc -S, gfx950): one bid evaluates
32 objects per lane with 817 VALU instructions (25.5 per evaluation, 16 of them the IEEE-sqrt expansion around
v_sqrt_f32), 16 ds_read2st64_b32 for the prices and 125 s_nop; the top-2 butterfly adds about 133 VALU instructions and
18 ds_bpermute_b32 per bid.  "evaluations" below are bids x N: every bid prices all N objects.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

VALU_PER_BID_K32 = 817 + 133          # bidding loop of emd_auction_kernel<32>: 32 evaluations per lane + the butterfly
CLOCK_GHZ = 2.4                       # MI355X peak engine clock
SIMDS = 256 * 4


def lidar_like(rng, n):
    """A spinning-sensor sweep: ranges 3 .. 70 m, 64 beams between -25 and +3 degrees, any azimuth (fp32 xyz)."""
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.choice(np.linspace(-25.0, 3.0, 64), n))
    r = np.minimum(3.0 + rng.exponential(12.0, n), 70.0)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)


def _lsa_seconds(pair):
    """One pair on the host: the fp32 cost matrix and linear_sum_assignment on it; returns (seconds, mean cost)."""
    from scipy.optimize import linear_sum_assignment
    x, y = pair
    t0 = time.perf_counter()
    d = x[:, None, :] - y[None, :, :]
    c = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    rows, cols = linear_sum_assignment(c)
    return time.perf_counter() - t0, float(c[rows, cols].astype(np.float64).sum() / len(x))


def host_baseline(pairs, workers):
    """Wall seconds per pair with `workers` processes busy, and each pair's optimal mean cost."""
    import multiprocessing as mp
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_lsa_seconds, pairs[:workers])          # start the workers and import scipy in each
        t0 = time.perf_counter()
        res = pool.map(_lsa_seconds, pairs, chunksize=1)
        wall = time.perf_counter() - t0
    return {"pairs": len(pairs), "workers": workers, "wall_seconds_per_pair": wall / len(pairs),
            "one_worker_seconds_per_pair_median": float(np.median([r[0] for r in res]))}, [r[1] for r in res]


def time_case(xs, ys, eps, reps):
    import torch
    from rangeldm_amd import _lib
    from rangeldm_amd.metrics import _pack
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    emd = torch.empty((len(xs), len(ys)), dtype=torch.float64, device=xp.device)
    bids = torch.empty((len(xs), len(ys)), dtype=torch.int32, device=xp.device)
    L, st = _lib.lib(), _lib.stream_ptr(xp.device)

    def run():
        _lib.check(L.rldm_emd_matrix(xp.data_ptr(), xo.data_ptr(), xk, len(xs), yp.data_ptr(), yo.data_ptr(), yk, len(ys),
                                     _lib.RLDM_EMD_RECT, eps, emd.data_ptr(), None, None, bids.data_ptr(), st), "rldm_emd_matrix")
        torch.cuda.synchronize()
    run()                                                # warm-up: code object load, allocator
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
        print(f"  {len(xs)} x {len(ys)}: repetition {len(ts)} took {ts[-1]:.3f} s", file=sys.stderr, flush=True)
    return ts, emd, bids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x64", "1000x1000"], help="NXxNY clouds per case")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=2.0 ** -7)
    ap.add_argument("--host-pairs", type=int, default=32, help="pairs (x_i, y_i) the host baseline solves")
    ap.add_argument("--host-workers", type=int, default=16)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in c.lower().split("x")) for c in a.cases]
    n_max = max(max(s) for s in shapes)
    rng = np.random.default_rng(1)
    xs_h = [lidar_like(rng, a.points) for _ in range(n_max)]
    ys_h = [lidar_like(rng, a.points) for _ in range(n_max)]
    # the host route first: its workers are forked, so the GPU must not be open yet
    hp = min(a.host_pairs, min(min(s) for s in shapes))
    host, host_opt = host_baseline([(xs_h[i], ys_h[i]) for i in range(hp)], a.host_workers)

    import torch
    dev = torch.device("cuda")
    xs = [torch.from_numpy(c).to(dev) for c in xs_h]
    ys = [torch.from_numpy(c).to(dev) for c in ys_h]
    out = {"device": torch.cuda.get_device_name(0), "points": a.points, "eps": a.eps, "host_linear_sum_assignment": host,
           "runs": []}
    for nx, ny in shapes:
        ts, emd, bids = time_case(xs[:nx], ys[:ny], a.eps, a.reps)
        pairs = nx * ny
        med = float(np.median(ts))
        mean_bids = float(bids.double().mean())
        diag = torch.diagonal(emd)[:hp].cpu().tolist()
        out["runs"].append({
            "case": f"{nx} x {ny} clouds of {a.points} points", "pairs": pairs, "reps": len(ts), "seconds": med,
            "seconds_min": min(ts), "seconds_max": max(ts), "us_per_pair": 1e6 * med / pairs,
            "bids_per_pair_mean": mean_bids, "bids_per_point_mean": mean_bids / a.points, "bids_per_pair_max": int(bids.max()),
            "evaluations_per_s": mean_bids * a.points * pairs / med,
            # a bid of the 2 048-point instance costs VALU_PER_BID_K32 wave instructions of 4 clocks each on one SIMD
            "valu_issue_fraction_k32": mean_bids * pairs * VALU_PER_BID_K32 * 4 / (med * SIMDS * CLOCK_GHZ * 1e9),
            "speedup_vs_host_16_workers": host["wall_seconds_per_pair"] / (med / pairs),
            "emd_minus_host_optimum_max": max(d - o for d, o in zip(diag, host_opt)),
            "emd_minus_host_optimum_min": min(d - o for d, o in zip(diag, host_opt)), "emd_mean": float(emd.mean())})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
