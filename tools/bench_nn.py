#!/usr/bin/env python3
"""Time the nearest-neighbour-with-index kernel (rangeldm_amd/csrc/nn_index.hip) on KITTI-size pairs, next to the search
without the index that every command already pays for and to the numpy statement on the host.

    python tools/bench_nn.py [--pairs 8 1000] [--points 60000] [--reps 5] [--workers 16] [--host-pairs 16]

Per pair count, two device legs, each the median [min, max] of --reps calls after one warm-up call, the calls of the two
legs alternating:

    nearest_neighbours  metrics.nearest_neighbours(return_hits=True) on the device clouds (packing, the int64 copies of the
                        indices and the call's own synchronisation included)
    nearest_sq_dists    metrics.nearest_sq_dists on the same pairs (chamfer_nn_kernel, unchanged)

and their ratio, the figure the kernel is judged by: what knowing WHICH point is nearest costs over knowing how far it is.
The two legs' d^2 are compared bit for bit.

The host leg, nearest_neighbours_host, is a brute force of n x m distances per pair and direction: about a minute of one
core for one KITTI-size pair.  It is therefore timed ONCE, on the first --host-pairs pairs, one per worker process
(--workers of them, forked before the GPU is opened), and reported as seconds per pair at that throughput; the ratio
host / device compares it with the device's seconds per pair at each pair count.  Its indices and hits are compared with the
device's on those pairs.  Clouds come from bench_voxel.py's restatement of bench_chamfer.py's generator (54-66 k points,
3-70 m; the target is the result with a fifth of the points dropped and the rest jittered by 3 cm).
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from bench_voxel import make_pairs, spread  # noqa: E402

_PAIRS = None           # (xs, ys) of the host leg: set before the pool forks, read by its workers


def _host_pair(p):
    from rangeldm_amd.metrics import nearest_neighbours_host
    xs, ys = _PAIRS
    return [part[0] for part in nearest_neighbours_host(xs[p:p + 1], ys[p:p + 1], return_hits=True)]


def time_host(xs, ys, workers):
    """(seconds of one pool.map over the pairs, their results): one pair per task."""
    global _PAIRS
    import rangeldm_amd.metrics  # noqa: F401  (imported before the fork: no worker pays for it inside the timed call)
    _PAIRS = (xs, ys)
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(abs, range(workers))                    # the workers exist before the clock starts
        t0 = time.perf_counter()
        parts = pool.map(_host_pair, range(len(xs)), chunksize=1)
        return time.perf_counter() - t0, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 1000])
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=16, help="pairs of the largest set the host leg runs (0: skip it)")
    a = ap.parse_args()
    sets = {n: make_pairs(n, a.points) for n in a.pairs}
    big = max(a.pairs)
    hp = min(a.host_pairs, big)
    host_s, host_parts = time_host(sets[big][0][:hp], sets[big][1][:hp], a.workers) if hp else (None, [])

    import torch
    from rangeldm_amd.metrics import nearest_neighbours, nearest_sq_dists
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "host_workers": a.workers, "host_pairs": hp,
           "host_seconds": host_s, "host_seconds_per_pair": host_s / hp if hp else None, "runs": []}
    for n in a.pairs:
        xs = [torch.from_numpy(c).to(dev) for c in sets[n][0]]
        ys = [torch.from_numpy(c).to(dev) for c in sets[n][1]]

        def run_index():
            res = nearest_neighbours(xs, ys, return_hits=True)
            torch.cuda.synchronize()
            return res

        def run_plain():
            res = nearest_sq_dists(xs, ys)
            torch.cuda.synchronize()
            return res

        full, plain = run_index(), run_plain()           # warm-up of both
        ti, tp = [], []
        for _ in range(a.reps):                          # alternating: a drift of the machine lands on both legs
            t0 = time.perf_counter()
            full = run_index()
            t1 = time.perf_counter()
            plain = run_plain()
            t2 = time.perf_counter()
            ti.append(t1 - t0)
            tp.append(t2 - t1)
        for side in (0, 1):
            if not torch.equal(torch.cat(full[2 * side]).view(torch.int32), torch.cat(plain[side]).view(torch.int32)):
                raise SystemExit(f"{n} pairs: the two searches' d^2 differ")
        if n == big:
            for p, want in enumerate(host_parts):
                got = [part[p].cpu().numpy() for part in full]
                if any(g.tobytes() != w.astype(g.dtype).tobytes() for g, w in zip(got, want)):
                    raise SystemExit(f"pair {p}: the device differs from nearest_neighbours_host")
        i, s = spread(ti), spread(tp)
        run = {"pairs": n, "points_per_pair": (sum(len(c) for c in sets[n][0]) + sum(len(c) for c in sets[n][1])) / n,
               "nearest_neighbours": i, "nearest_sq_dists": s, "index_over_plain": i["seconds"] / s["seconds"],
               "index_over_plain_min": i["seconds_min"] / s["seconds_max"], "index_over_plain_max": i["seconds_max"] / s["seconds_min"],
               "d2_bit_equal": True, "mean_hits_max": float(np.mean([int(h.max()) for h in full[5][:64]]))}
        if hp:
            run["host_over_index_per_pair"] = (host_s / hp) / (i["seconds"] / n)
            run["equals_host"] = n == big or None
        out["runs"].append(run)
        del xs, ys, full, plain
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
