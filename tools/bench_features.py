#!/usr/bin/env python3
"""Time precision / recall / density / coverage (metrics.prdc) and the kernel distance (metrics.kernel_distance;
rangeldm_amd/csrc/feature_metrics.hip) on synthetic activations of d = 4 096 values, n = 1 000 and n = 10 000 samples per
set: each call repeated five times after one warm-up call and reported as median [min, max].  In the same process:

  (a) gram_f64 alone on the same operands -- the floor: a scan does the same products.  prdc is four scans and the kernel
      distance three, so "scan_over_gram" is (call time / scans) / (time of one Gram product).
  (b) the materialising route: gram_f64 into (n, n) matrices, then torch.topk and comparisons (prdc) or elementwise kernel
      and row sums (kernel distance).  Its scores must equal the scan's.
  (c) the numpy statements (prdc_host, kernel_distance_host) on 16 host threads, once.

and the peak device bytes each route allocates beyond the two operand sets: torch's allocator peak, plus -- for the scan,
whose workspace comes from the stream's pool inside the library -- the workspace computed from the shapes the way
include/rangeldm_hip.h states it.

    python tools/bench_features.py [--n 1000 10000] [--d 4096] [--k 5] [--reps 5] [--skip-host]

Time is a host clock around calls on device-resident fp64 inputs that end in a synchronise (every route reads its counts
or sums back).  Nothing here is a pass / fail threshold.
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


def timed(fn, reps):
    fn()                                                 # warm-up: code object load, allocator pools
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"seconds": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "reps": len(ts)}


def scan_workspace_bytes(n_a, n_b, k1, counts, poly, same):
    """What one rldm_feature_scan_f64 call takes from the stream's pool: the norms and, with more than one column chunk,
    every output once per chunk."""
    from rangeldm_amd.metrics import feature_scan_column_chunk
    chunks = -(-n_b // feature_scan_column_chunk(n_b))
    per = chunks * n_a if chunks > 1 else 0
    return 8 * (n_a + (0 if same else n_b) + per * (k1 + 1 + (1 if poly else 0))) + 4 * per * counts + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 10000], help="samples per set")
    ap.add_argument("--d", type=int, default=4096, help="values per sample")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="do not run the numpy statements")
    a = ap.parse_args()

    import torch
    from rangeldm_amd import metrics as M
    dev = torch.device("cuda")
    k = a.k
    out = {"device": torch.cuda.get_device_name(0), "dims": a.d, "k": k, "sizes": []}

    def materialised_d2(g, s_p, s_q):
        """(n, n) squared distances the way the scan defines them, from a whole Gram matrix and the two sets' norms."""
        return ((s_p[:, None] + s_q[None, :]) - 2.0 * g).clamp_(min=0.0)

    def prdc_materialised(real, fake):
        n, m = real.shape[0], fake.shape[0]
        g_rr, g_ff = M.gram_f64(real, real), M.gram_f64(fake, fake)
        s_r, s_f = torch.diagonal(g_rr).clone(), torch.diagonal(g_ff).clone()
        r_real = torch.topk(materialised_d2(g_rr, s_r, s_r), k + 1, dim=1, largest=False).values[:, k]
        r_fake = torch.topk(materialised_d2(g_ff, s_f, s_f), k + 1, dim=1, largest=False).values[:, k]
        del g_rr, g_ff
        d2 = materialised_d2(M.gram_f64(real, fake), s_r, s_f)
        inside = d2 < r_real[:, None]
        return {"precision": int(inside.any(0).sum()) / m, "recall": int((d2 < r_fake[None, :]).any(1).sum()) / n,
                "density": int(inside.sum()) / (k * m), "coverage": int((d2.min(1).values < r_real).sum()) / n}

    def krd_materialised(x, y):
        import math
        n1, n2, d = x.shape[0], y.shape[0], x.shape[1]
        sums = []
        for p, q, skip in ((x, x, True), (y, y, True), (x, y, False)):
            t = M.gram_f64(p, q) / d + 1.0
            kappa = t * t * t
            if skip:
                kappa.fill_diagonal_(0.0)
            sums.append(math.fsum(kappa.sum(1).cpu().tolist()))
        return sums[0] / (n1 * (n1 - 1)) + sums[1] / (n2 * (n2 - 1)) - (2.0 * sums[2]) / (n1 * n2)

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    for n in a.n:
        x, y = synthetic(n, a.d, 1)
        fake, real = torch.from_numpy(x).to(dev).double(), torch.from_numpy(y).to(dev).double()
        flop = 2.0 * n * n * a.d
        res = {}

        def gram_only():
            M.gram_f64(real, fake)
            torch.cuda.synchronize()

        def scan_only():
            M.feature_scan(real, fake, k=k).min_sq.sum().item()

        gram = timed(gram_only, a.reps)
        gram.update(tflops=flop / gram["seconds"] / 1e12, fraction_of_fp64_mfma_rate=flop / gram["seconds"] / 1e12 / FP64_MFMA_TFLOPS)
        one = timed(scan_only, a.reps)
        one.update(tflops=flop / one["seconds"] / 1e12, scan_over_gram=one["seconds"] / gram["seconds"])
        scan_p = timed(lambda: res.__setitem__("prdc", M.prdc(real, fake, k=k)), a.reps)
        scan_k = timed(lambda: res.__setitem__("krd", M.kernel_distance(fake, real)), a.reps)
        mat_p = timed(lambda: res.__setitem__("prdc_m", prdc_materialised(real, fake)), a.reps)
        mat_k = timed(lambda: res.__setitem__("krd_m", krd_materialised(fake, real)), a.reps)
        scan_p["scan_over_gram"] = scan_p["seconds"] / 4 / gram["seconds"]
        scan_k["scan_over_gram"] = scan_k["seconds"] / 3 / gram["seconds"]
        # peak bytes beyond the operands: torch's allocator, plus the scan's pool workspace (the largest of prdc's four scans)
        scan_p["peak_bytes"] = peak_of(lambda: M.prdc(real, fake, k=k)) + max(
            scan_workspace_bytes(n, n, k + 1, 0, False, True), scan_workspace_bytes(n, n, 0, 2, False, False))
        scan_k["peak_bytes"] = peak_of(lambda: M.kernel_distance(fake, real)) + scan_workspace_bytes(n, n, 0, 0, True, False)
        mat_p["peak_bytes"] = peak_of(lambda: prdc_materialised(real, fake))
        mat_k["peak_bytes"] = peak_of(lambda: krd_materialised(fake, real))
        size = {"n": n, "gram_f64": gram, "feature_scan_k": one, "prdc": {"scan": scan_p, "materialised": mat_p, "value": res["prdc"],
                                                                            "routes_equal": res["prdc"] == res["prdc_m"]},
                "kernel_distance": {"scan": scan_k, "materialised": mat_k, "value": res["krd"],
                                    "materialised_minus_scan": res["krd_m"] - res["krd"]}}
        print(json.dumps(size), file=sys.stderr, flush=True)   # (the device half, before the long host half)
        if not a.skip_host:
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            t0 = time.perf_counter()
            host_p = M.prdc_host(y64, x64, k=k)
            t1 = time.perf_counter()
            host_k = M.kernel_distance_host(x64, y64)
            t2 = time.perf_counter()
            threads = int(os.environ["OMP_NUM_THREADS"])
            size["prdc"]["host"] = {"seconds": t1 - t0, "threads": threads, "equal_to_scan": host_p == res["prdc"]}
            size["kernel_distance"]["host"] = {"seconds": t2 - t1, "threads": threads, "host_minus_scan": host_k - res["krd"]}
        out["sizes"].append(size)
        del fake, real
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
