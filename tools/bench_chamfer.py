#!/usr/bin/env python3
"""Time the Chamfer-distance kernel (rangeldm_amd/csrc/chamfer.hip) at the reference's evaluation size (1000 pairs of
KITTI-360-size clouds, ldm/convert_vae.py:262-271) and one 65 536 x 65 536 pair, price it against the fp32 VALU issue
rate, and time a same-process host baseline (scipy cKDTree, 16 workers).

    python tools/bench_chamfer.py [--pairs 1000] [--points 60000] [--host-pairs 8] [--matrix NX NY POINTS]

--matrix NX NY POINTS adds the all-pairs matrix (rldm_chamfer_matrix, both directions) between NX and NY clouds of POINTS
points, and the same cloud size through the pair entry point on a --matrix-block x --matrix-block sub-block with every cloud
replicated once per partner (what the matrix would cost without the kernel's reuse); five repetitions each, spread reported.

Instruction count per evaluation, read from the ISA of chamfer_nn_kernel's inner loop (hipcc --save-temps, gfx950): one
iteration handles 4 targets x 8 queries = 32 evaluations with 80 v_pk_add_f32 + 48 v_pk_mul_f32 + 16 v_min3_f32 +
3 v_mov_b32 = 147 VALU instructions, i.e. 4.59 per evaluation (the packed forms do two fp32 operations per lane).
The issue rate is 16 lanes x 4 SIMDs x 256 CUs per clock: a wave64 VALU instruction occupies its SIMD for 4 clocks.
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
import torch  # noqa: E402

VALU_PER_EVAL = 147 / 32
CLOCK_GHZ = 2.4                       # MI355X peak engine clock
LANE_ISSUE_PER_S = 256 * 4 * 16 * CLOCK_GHZ * 1e9


def kitti_like(g, n, device):
    r = torch.rand(n, generator=g, device=device, dtype=torch.float64) * 67.0 + 3.0
    az = (torch.rand(n, generator=g, device=device, dtype=torch.float64) * 2.0 - 1.0) * np.pi
    el = torch.rand(n, generator=g, device=device, dtype=torch.float64) * 0.46 - 0.43
    return torch.stack([r * el.cos() * az.cos(), r * el.cos() * az.sin(), r * el.sin() + 1.7], 1).float()


def time_nn(xs, ys, reps):
    """Seconds per call of rldm_chamfer_nn + rldm_chamfer_mean on pre-packed clouds (median of `reps`)."""
    from rangeldm_amd import _lib
    from rangeldm_amd.metrics import _pack
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    xd = torch.empty(xp.shape[0], device=xp.device)
    yd = torch.empty(yp.shape[0], device=xp.device)
    xm = torch.empty(len(xs), dtype=torch.float64, device=xp.device)
    ym = torch.empty_like(xm)
    L, st = _lib.lib(), _lib.stream_ptr(xp.device)

    def run():
        _lib.check(L.rldm_chamfer_nn(xp.data_ptr(), xo.data_ptr(), xk, yp.data_ptr(), yo.data_ptr(), yk, len(xs),
                                     xd.data_ptr(), yd.data_ptr(), st), "rldm_chamfer_nn")
        _lib.check(L.rldm_chamfer_mean(xd.data_ptr(), xo.data_ptr(), yd.data_ptr(), yo.data_ptr(), len(xs), xm.data_ptr(),
                                       ym.data_ptr(), st), "rldm_chamfer_mean")
        torch.cuda.synchronize()
    run()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float((xm + ym).mean())


def time_matrix(xs, ys, reps):
    """Seconds per call of rldm_chamfer_matrix on pre-packed sets (every one of `reps`, after one warm-up call)."""
    from rangeldm_amd import _lib
    from rangeldm_amd.metrics import _pack
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    xy = torch.empty((len(xs), len(ys)), dtype=torch.float64, device=xp.device)
    yx = torch.empty_like(xy)
    L, st = _lib.lib(), _lib.stream_ptr(xp.device)

    def run():
        _lib.check(L.rldm_chamfer_matrix(xp.data_ptr(), xo.data_ptr(), xk, len(xs), yp.data_ptr(), yo.data_ptr(), yk, len(ys), 0,
                                         xy.data_ptr(), yx.data_ptr(), st), "rldm_chamfer_matrix")
        torch.cuda.synchronize()
    run()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return ts, xy + yx


def spread(ts, evals):
    med = float(np.median(ts))
    return {"seconds": med, "seconds_min": min(ts), "seconds_max": max(ts), "reps": len(ts), "evals_per_s": evals / med,
            "evals_per_s_spread": [evals / max(ts), evals / min(ts)],
            "valu_issue_fraction": evals / med * VALU_PER_EVAL / LANE_ISSUE_PER_S}


def matrix_report(g, nx, ny, points, block, dev):
    xs = [kitti_like(g, points, dev) for _ in range(nx)]
    ys = [kitti_like(g, points, dev) for _ in range(ny)]
    ts, cd = time_matrix(xs, ys, 5)
    out = {"matrix": {"case": f"{nx} x {ny} clouds of {points} pts, both directions", **spread(ts, 2.0 * nx * ny * points * points),
                      "cd_mean": float(cd.mean())}}
    # the same clouds through the pair entry point: a block x block corner of the matrix, every cloud once per partner
    bx, by = min(block, nx), min(block, ny)
    px = [xs[i] for i in range(bx) for _ in range(by)]
    py = [ys[j] for _ in range(bx) for j in range(by)]
    ts = [time_nn(px, py, 1)[0] for _ in range(5)]
    out["pair_path_block"] = {"case": f"{bx} x {by} corner as {bx * by} pairs of {points} pts",
                              **spread(ts, 2.0 * bx * by * points * points)}
    out["pair_path_block"]["seconds_for_whole_matrix"] = out["pair_path_block"]["seconds"] * (nx * ny) / (bx * by)
    return out


def host_seconds_per_pair(xs, ys):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    for x, y in zip(xs, ys):
        x, y = x.double().cpu().numpy(), y.double().cpu().numpy()
        cKDTree(y).query(x, k=1, workers=16)
        cKDTree(x).query(y, k=1, workers=16)
    return (time.perf_counter() - t0) / len(xs)


def report(name, xs, ys, reps):
    evals = 2.0 * sum(x.shape[0] * y.shape[0] for x, y in zip(xs, ys))
    sec, cd = time_nn(xs, ys, reps)
    rate = evals / sec
    return {"case": name, "pairs": len(xs), "seconds": sec, "ms_per_pair": 1e3 * sec / len(xs), "evals_per_s": rate,
            "valu_issue_fraction": rate * VALU_PER_EVAL / LANE_ISSUE_PER_S, "cd": cd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--host-pairs", type=int, default=8, help="pairs the cKDTree baseline times (per-pair cost is reported)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--matrix", type=int, nargs=3, metavar=("NX", "NY", "POINTS"), default=None,
                    help="also time the all-pairs matrix between NX and NY clouds of POINTS points")
    ap.add_argument("--matrix-block", type=int, default=64, help="side of the sub-block timed through the pair entry point")
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    sizes = torch.randint(a.points - a.points // 10, a.points + a.points // 10 + 1, (2 * a.pairs,), generator=g, device=dev)
    sizes = sizes.cpu().tolist()
    xs = [kitti_like(g, n, dev) for n in sizes[:a.pairs]]
    ys = [kitti_like(g, n, dev) for n in sizes[a.pairs:]]
    big_x, big_y = [kitti_like(g, 65536, dev)], [kitti_like(g, 65536, dev)]
    out = {"device": torch.cuda.get_device_name(0), "valu_per_eval": VALU_PER_EVAL, "clock_ghz_assumed": CLOCK_GHZ,
           "runs": [report(f"{a.pairs} pairs ~{a.points} pts", xs, ys, a.reps),
                    report("1 pair 65536 x 65536", big_x, big_y, a.reps)]}
    host = host_seconds_per_pair(xs[:a.host_pairs], ys[:a.host_pairs])
    out["host_ckdtree_16w_ms_per_pair"] = 1e3 * host
    out["speedup_vs_host"] = host / (out["runs"][0]["seconds"] / a.pairs)
    if a.matrix:
        out.update(matrix_report(g, *a.matrix, a.matrix_block, dev))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
