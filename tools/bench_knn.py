#!/usr/bin/env python3
"""Time the K-nearest-neighbour kernel (rangeldm_amd/csrc/knn.hip) and what stands on it on KITTI-size pairs, next to the
nearest-neighbour search every command already pays for and to a k-d tree on the host.

    python tools/bench_knn.py [--pairs 8 1000] [--points 60000] [--reps 5] [--workers 16] [--host-pairs 16]
                              [--legs search normals plane chain host] [--step-timeout 900]

Every leg runs in a child process of its own under --step-timeout seconds (the parent never opens the GPU), and the first leg
that fails ends the run.  A timed figure is the median [min, max] of --reps calls after one warm-up call; where two calls are
compared they alternate.  Clouds come from bench_voxel.py's generator, as in bench_nn.py (54-66 k points, 3-70 m; the target is
the result with a fifth of the points dropped and the rest jittered by 3 cm).

    search   per pair count: self_neighbours of the result clouds at K = 8, 16, 32 and knn_points(result, target) at K = 1,
             each alternating with nearest_neighbours on the same pairs, of which ONE direction's share (half) is the
             comparison point: what keeping K neighbours costs over keeping one
    normals  estimate_normals at K = 16 against self_neighbours at K = 16 alone: the difference is the PCA on given indices
    plane    plane_scores at K = 16 against pair_scores
    chain    what the insertion chain costs, without a switch in the kernel: knn_points of queries that all sit within a
             centimetre of one point against a target cloud sorted by distance from that point, ascending (after the first K
             targets nothing is inserted: the distance loop alone), descending (every target is inserted: the chain at its
             worst) and shuffled, per K; the real clouds' self_neighbours of the search leg lie between the first two
    host     scipy.spatial.cKDTree(cloud).query(cloud, k=K + 1) at K = 16, timed once on --host-pairs clouds, one per worker
             process, and reported as seconds per cloud at that throughput
"""
import argparse
import json
import multiprocessing as mp
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from bench_voxel import make_pairs, spread  # noqa: E402

LEGS = ("search", "normals", "plane", "chain", "host")
_CLOUDS = None          # the host leg's clouds: set before the pool forks, read by its workers


def alternate(fa, fb, reps):
    """Medians of two calls timed in turn (a drift of the machine lands on both), after one warm-up of each."""
    import torch

    def timed(f):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    timed(fa), timed(fb)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return spread(ta), spread(tb)


def _device_pairs(n, points):
    import torch
    xs, ys = make_pairs(n, points)
    dev = torch.device("cuda")
    return [torch.from_numpy(c).to(dev) for c in xs], [torch.from_numpy(c).to(dev) for c in ys]


def leg_search(a):
    from rangeldm_amd.metrics import knn_points, nearest_neighbours, self_neighbours
    runs = []
    for n in a.pairs:
        xs, ys = _device_pairs(n, a.points)
        run = {"pairs": n}
        for K in (8, 16, 32, 1):
            call = (lambda: knn_points(xs, ys, 1)) if K == 1 else (lambda: self_neighbours(xs, K))
            k, nn = alternate(call, lambda: nearest_neighbours(xs, ys), a.reps)
            half = nn["seconds"] / 2
            run["knn_points_k1" if K == 1 else f"self_neighbours_k{K}"] = {
                **k, "nearest_neighbours": nn, "over_one_direction": k["seconds"] / half,
                "over_one_direction_min": k["seconds_min"] / (nn["seconds_max"] / 2),
                "over_one_direction_max": k["seconds_max"] / (nn["seconds_min"] / 2)}
        d2, idx = knn_points(xs[:8], ys[:8], 1)
        xd, xi, _, _ = nearest_neighbours(xs[:8], ys[:8])
        run["k1_equals_nearest_neighbours"] = all(bool((u[:, 0].view(xd[0].dtype) == v).all()) and bool((i[:, 0] == j).all())
                                                  for u, v, i, j in zip(d2, xd, idx, xi))
        runs.append(run)
        del xs, ys
    return runs


def leg_normals(a):
    from rangeldm_amd.metrics import estimate_normals, self_neighbours
    runs = []
    for n in a.pairs:
        xs, _ = _device_pairs(n, a.points)
        full, search = alternate(lambda: estimate_normals(xs, 16), lambda: self_neighbours(xs, 16), a.reps)
        runs.append({"pairs": n, "estimate_normals_k16": full, "self_neighbours_k16": search,
                     "pca_seconds": full["seconds"] - search["seconds"]})
        del xs
    return runs


def leg_plane(a):
    from rangeldm_amd.metrics import pair_scores, plane_scores
    runs = []
    for n in a.pairs:
        xs, ys = _device_pairs(n, a.points)
        plane, pair = alternate(lambda: plane_scores(xs, ys, 16), lambda: pair_scores(xs, ys), a.reps)
        runs.append({"pairs": n, "plane_scores_k16": plane, "pair_scores": pair, "plane_over_pair": plane["seconds"] / pair["seconds"]})
        del xs, ys
    return runs


def leg_chain(a):
    import torch
    from rangeldm_amd.metrics import knn_points
    n = min(a.pairs)
    xs, _ = make_pairs(n, a.points)
    rng = np.random.default_rng(2)
    centre = np.float32([10.0, 5.0, -1.0])
    order = [np.argsort(((c - centre) ** 2).sum(1)) for c in xs]
    dev = torch.device("cuda")
    put = lambda cs: [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cs]      # noqa: E731
    queries = put([(centre + 0.005 * rng.standard_normal((len(c), 3))).astype(np.float32) for c in xs])
    up, down = put([c[o] for c, o in zip(xs, order)]), put([c[o[::-1]] for c, o in zip(xs, order)])
    mixed = put([c[rng.permutation(len(c))] for c in xs])
    out = {"pairs": n}
    for K in (8, 16, 32):
        asc, desc = alternate(lambda: knn_points(queries, up, K), lambda: knn_points(queries, down, K), a.reps)
        mix, _ = alternate(lambda: knn_points(queries, mixed, K), lambda: None, a.reps)
        out[f"k{K}"] = {"ascending": asc, "descending": desc, "shuffled": mix,
                        "descending_over_ascending": desc["seconds"] / asc["seconds"],
                        "shuffled_over_ascending": mix["seconds"] / asc["seconds"]}
    return out


def _tree(i):
    from scipy.spatial import cKDTree
    c = _CLOUDS[i].astype(np.float64)
    d, j = cKDTree(c).query(c, k=17)
    return float(d[:, 1:].mean())


def leg_host(a):
    global _CLOUDS
    _CLOUDS = make_pairs(a.host_pairs, a.points)[0]
    with mp.get_context("fork").Pool(a.workers) as pool:
        pool.map(abs, range(a.workers))                  # the workers exist before the clock starts
        t0 = time.perf_counter()
        pool.map(_tree, range(len(_CLOUDS)), chunksize=1)
        s = time.perf_counter() - t0
    return {"workers": a.workers, "clouds": len(_CLOUDS), "k": 16, "seconds": s, "seconds_per_cloud": s / len(_CLOUDS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 1000])
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=16, help="clouds the k-d tree leg runs")
    ap.add_argument("--legs", nargs="+", choices=LEGS, default=list(LEGS))
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a leg's process may take")
    ap.add_argument("--leg", choices=LEGS, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:                                            # a child: one leg, one JSON line
        print(json.dumps({a.leg: globals()["leg_" + a.leg](a)}))
        return
    out = {}
    for leg in a.legs:
        argv = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--pairs", *map(str, a.pairs), "--points", str(a.points),
                "--reps", str(a.reps), "--workers", str(a.workers), "--host-pairs", str(a.host_pairs)]
        done = subprocess.run(argv, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
        if done.returncode != 0:
            print(json.dumps(out, indent=1))
            raise SystemExit(f"leg {leg} ended with status {done.returncode}: nothing more is started")
        out.update(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps({leg: out[leg]}), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
