#!/usr/bin/env python3
"""Time the Frechet distance over dumped activations (rangeldm_amd/csrc/frechet.hip, metrics.frechet_distance) on synthetic
activations, n1 = n2 = 1 000 samples of d = 4 096 values: the device call repeated five times after one warm-up call and
reported as median [min, max], with the Jacobi sweeps and launches, and the Gram kernel alone (its share of the call and its
fraction of the fp64 MFMA rate); and, in the same session, the route it replaces: np.mean / np.cov and scipy.linalg.sqrtm
of the 4 096 x 4 096 product on 16 host threads (the formulation of the reference's calculate_frechet_distance).

    python tools/bench_frechet.py [--n 1000] [--d 4096] [--reps 5] [--skip-host]

Time is a host clock around rldm_frechet_distance / rldm_gram_f64 on device-resident fp64 inputs, each followed by a
synchronise (rldm_frechet_distance synchronises the stream itself: it reads the rotation count once per sweep).
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")                      # the host baseline's thread count, fixed before numpy loads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FP64_MFMA_TFLOPS = 78.6               # MI355X peak fp64 matrix rate (vendor specification)


def synthetic(n, d, seed):
    """Two sets of activations with per-value scales and a mean shift between them (fp32 values, as dumped files hold)."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.2, 3.0, d)
    x = (rng.normal(0.0, 1.0, (n, d)) * scale).astype(np.float32)
    y = (rng.normal(0.1, 1.1, (n, d)) * scale).astype(np.float32)
    return x, y


def host_reference_formulation(x, y):
    """mean / cov / sqrtm, the way the reference computes it; returns (value, seconds by stage)."""
    from scipy import linalg
    t0 = time.perf_counter()
    mu1, mu2 = np.mean(x, axis=0), np.mean(y, axis=0)
    s1, s2 = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    t1 = time.perf_counter()
    print(f"  host: mean / cov took {t1 - t0:.2f} s; sqrtm of a {s1.shape[0]} x {s1.shape[0]} product ...", file=sys.stderr,
          flush=True)
    covmean = linalg.sqrtm(s1.dot(s2))
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    t2 = time.perf_counter()
    diff = mu1 - mu2
    value = float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(covmean)))
    return value, {"mean_cov_seconds": t1 - t0, "sqrtm_seconds": t2 - t1, "seconds": time.perf_counter() - t0}


def timed(fn, reps):
    fn()                                                 # warm-up: code object load, allocator pools
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"seconds": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "reps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="samples per set")
    ap.add_argument("--d", type=int, default=4096, help="values per sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="do not run the mean / cov / sqrtm baseline")
    a = ap.parse_args()
    x, y = synthetic(a.n, a.d, 1)

    import torch
    from rangeldm_amd import _lib
    from rangeldm_amd import metrics as M
    dev = torch.device("cuda")
    dx, dy = torch.from_numpy(x).to(dev).double(), torch.from_numpy(y).to(dev).double()
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    out5 = (M.C.c_double * 5)()
    gram = torch.empty((a.n, a.n), dtype=torch.float64, device=dev)

    def call():
        M._frechet_check(L.rldm_frechet_distance(dx.data_ptr(), a.n, dy.data_ptr(), a.n, a.d, out5, st), "rldm_frechet_distance")
        torch.cuda.synchronize()

    def gram_only():
        _lib.check(L.rldm_gram_f64(dx.data_ptr(), a.n, dy.data_ptr(), a.n, a.d, gram.data_ptr(), st), "rldm_gram_f64")
        torch.cuda.synchronize()

    whole = timed(call, a.reps)
    sweeps = int(L.rldm_frechet_last_sweeps())
    g = timed(gram_only, a.reps)
    cpad = a.n + (a.n & 1)
    flop = 2.0 * a.n * a.n * a.d
    out = {"device": torch.cuda.get_device_name(0), "n1": a.n, "n2": a.n, "dims": a.d, "frd": out5[0],
           "terms": {"mean_sq": out5[1], "tr1": out5[2], "tr2": out5[3], "tr_sqrt": out5[4]},
           "frechet_distance": whole, "sweeps": sweeps, "jacobi_launches": sweeps * (cpad - 1),
           "launches": sweeps * (cpad - 1) + 10,         # + finite x2, mean x2, centre x2, totals, Gram, transpose, norms
           "gram": {**g, "share_of_call": g["seconds"] / whole["seconds"], "tflops": flop / g["seconds"] / 1e12,
                    "fraction_of_fp64_mfma_rate": flop / g["seconds"] / 1e12 / FP64_MFMA_TFLOPS},
           "us_per_launch_outside_gram": 1e6 * (whole["seconds"] - g["seconds"]) / (sweeps * (cpad - 1) + 9)}
    print(json.dumps(out), file=sys.stderr, flush=True)  # (the device half, before the long host half)
    if not a.skip_host:
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        value, host = host_reference_formulation(x64, y64)
        host.update(threads=int(os.environ["OMP_NUM_THREADS"]), value=value)
        t0 = time.perf_counter()
        gs = M.frechet_distance_host(x64, y64)
        out["host_mean_cov_sqrtm"] = host
        out["host_gram_svd"] = {"seconds": time.perf_counter() - t0, "value": gs}
        scale = out5[2] + out5[3]
        out["device_minus_host_gram_svd_over_traces"] = (out5[0] - gs) / scale
        out["device_minus_host_sqrtm_over_traces"] = (out5[0] - value) / scale
        out["speedup_vs_host_sqrtm"] = host["seconds"] / whole["seconds"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
