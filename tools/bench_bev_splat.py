#!/usr/bin/env python3
"""Time the order-fixed BEV splat against the atomic one (rangeldm_amd/csrc/lidar.hip: rldm_lidar_to_voxel against
rldm_lidar_to_voxel_ordered) at batch 8, 1024 x 64, the KITTI-360 tables and the reference's [1, 512, 512] volume over +-51.2 m.

    python tools/bench_bev_splat.py [--batch 8] [--calls 5] [--warmup 3]

Two inputs, drawn with rangeldm_amd/synth.py's named streams:
  sweep     every pixel's range uniform in 1 .. 60 m, remission uniform in 0 .. 1
  crowded   the same sweep with every third pixel set to decode to 0 .. 5 cm: those pixels all vote into the few cells under the
            sensor, whose sums the ordered splat adds one vote after the other
Per input the two calls alternate (atomic, ordered, atomic, ...); each call is timed on its own with device events after a shared
warm-up: median [min, max] of --calls calls.  One JSON line per input, with the ordered splat's time as a multiple of the atomic
one's in the same run, the largest raw density of a cell (every vote weighs at most 1: a lower bound of the votes that cell takes)
and whether two ordered calls returned the same bits."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def tri(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20240310)
    a = ap.parse_args()
    from rangeldm_amd import _lib
    from rangeldm_amd.range_image import point_cloud_to_range_image_KITTI
    from rangeldm_amd.synth import uniform
    _lib.require_gpu()
    B, W, H = a.batch, 1024, 64
    t = point_cloud_to_range_image_KITTI(width=W, grid_sizes=[1, 512, 512], pc_range=[-51.2, -51.2, -3., 51.2, 51.2, 1.])
    metres = 1.0 + 59.0 * uniform(a.seed, "bev_splat/range", (B, W, H))
    rem = uniform(a.seed, "bev_splat/remission", (B, W, H)).astype(np.float32)
    near = 0.05 * uniform(a.seed, "bev_splat/near", (B, W, H))
    third = (np.arange(W * H) % 3 == 0).reshape(1, W, H)
    inputs = {"sweep": metres, "crowded": np.where(third, near, metres)}
    for name, m in inputs.items():
        img = torch.from_numpy(np.stack([((m - t.mean) / t.std).astype(np.float32), rem], 1)).cuda()
        calls = {"atomic": lambda: t.to_voxel(img), "ordered": lambda: t.to_voxel(img, ordered=True)}
        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.calls):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        _, (_, raw) = t.to_voxel_train(img)
        va, vo = calls["atomic"](), calls["ordered"]()
        out = {"input": name, "batch": B, "image": [W, H], "grid": [1, 512, 512], "calls": a.calls,
               "atomic_ms": tri(ms["atomic"]), "ordered_ms": tri(ms["ordered"]),
               "ordered_over_atomic": float(np.median(ms["ordered"]) / np.median(ms["atomic"])),
               "largest_cell_density": float(raw[:, 0].max()), "occupied_cells_per_image": float((raw[:, 0] > 0).sum() / B),
               "largest_difference_ordered_atomic": float((va - vo).abs().max()),
               "ordered_repeats_its_bits": bool(torch.equal(vo, calls["ordered"]()))}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
