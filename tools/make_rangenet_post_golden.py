#!/usr/bin/env python3
"""Write tests/golden/rangenet_post.npz: what the reference's LaserScan and its KNN post-processing compute, recorded on the CPU.

    python tools/make_rangenet_post_golden.py --reference /path/to/RangeLDM [--out tests/golden/rangenet_post.npz]

The reference's own modules do the computing: modules/kittiparser.py (LaserScan) and postproc/KNN.py are loaded by path
(KNN.py does `import __init__ as booger`: an empty module of that name is put into sys.modules first).  Only arrays are written.

Keys
  cases                                      how many clouds
  c{i}_hw, c{i}_points, c{i}_remission       the image size and the seeded cloud (rangenet.synthetic_cloud: pairwise distinct depths)
  c{i}_proj_x, _proj_y, _unproj_range, _proj_range      LaserScan's per-point pixels and depth, and its range image
  c{i}_argmax                                a seeded label image, constant over 4 x 8 pixel blocks, classes 0..19 (uint8)
  params                                     (P, 4) float64: knn, search, sigma, cutoff
  w{j}                                       float32 (search^2,): 1 - get_gaussian_kernel(search, sigma) of params[j]
  c{i}_knn{j}                                uint8 (N,): KNN(params[j], 20).forward(...) of cloud i

The tool asserts that the recorded input is tie-free, so that the comparison with any restatement is exact and without
exclusions: no two points of one pixel share a depth, and no point has a finite, in-cutoff tie between its knn-th and its next
distance (the only place torch.topk's order among equals could show).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rangeldm_amd import rangenet as R                   # noqa: E402

TRAIN = "metrics/rangenetpp/lidar_bonnetal_master/train"
CASES = ((42, 3000, (16, 64)), (41, 6000, (8, 128)))     # seed, points asked for, (H, W)
PARAMS = ((5, 5, 1.0, 1.0), (3, 3, 0.5, 0.5), (7, 7, 2.0, 2.0))
NCLASSES = R.NUM_CLASSES


def load_module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blocky_labels(seed, H, W):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, NCLASSES, ((H + 3) // 4, (W + 7) // 8))
    return np.repeat(np.repeat(blocks, 4, 0), 8, 1)[:H, :W].astype(np.uint8)


def window_distances(proj_range, unproj_range, px, py, search, w):
    """(N, search^2) distances by the rules of rangenet.knn_labels_host (only used to look for ties)."""
    pad = search // 2
    rp = np.pad(proj_range, pad)
    d = np.empty((px.shape[0], search * search), np.float32)
    for k in range(search * search):
        dy, dx = divmod(k, search)
        e = rp[py + dy, px + dx]
        e = np.where(e < 0, np.float32(np.inf), e)
        if k == (search * search - 1) // 2:
            e = unproj_range
        d[:, k] = np.abs(e - unproj_range) * w[k]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rangenet_post.npz"))
    a = ap.parse_args()
    sys.modules.setdefault("__init__", types.ModuleType("__init__"))
    kp = load_module(os.path.join(a.reference, TRAIN, "tasks/semantic/modules/kittiparser.py"), "ref_kittiparser")
    knn_mod = load_module(os.path.join(a.reference, TRAIN, "tasks/semantic/postproc/KNN.py"), "ref_knn")

    out = {"cases": np.int64(len(CASES)), "params": np.asarray(PARAMS, dtype=np.float64)}
    for j, (knn, search, sigma, cutoff) in enumerate(PARAMS):
        out[f"w{j}"] = (1 - knn_mod.get_gaussian_kernel(search, sigma, 1)).reshape(-1).numpy().astype(np.float32)
    for i, (seed, n, (H, W)) in enumerate(CASES):
        pts, rem = R.synthetic_cloud(seed, n=n)
        scan = kp.LaserScan(project=True, H=H, W=W, fov_up=3.0, fov_down=-25.0)
        scan.set_points(pts, rem)
        px, py = scan.proj_x.astype(np.int32), scan.proj_y.astype(np.int32)
        depth = scan.unproj_range.astype(np.float32)
        pix_depth = np.stack([py.astype(np.int64) * W + px, depth.view(np.int32).astype(np.int64)], 1)
        assert np.unique(pix_depth, axis=0).shape[0] == pts.shape[0], "two points of one pixel share a depth"
        argmax = blocky_labels(seed, H, W)
        out.update({f"c{i}_hw": np.asarray([H, W], np.int64), f"c{i}_points": pts, f"c{i}_remission": rem, f"c{i}_proj_x": px,
                    f"c{i}_proj_y": py, f"c{i}_unproj_range": depth, f"c{i}_proj_range": scan.proj_range.astype(np.float32),
                    f"c{i}_argmax": argmax})
        plain = argmax[py, px]
        for j, (knn, search, sigma, cutoff) in enumerate(PARAMS):
            d = np.sort(window_distances(scan.proj_range, depth, px, py, search, out[f"w{j}"]), axis=1)
            if knn < search * search:
                tie = (d[:, knn - 1] == d[:, knn]) & np.isfinite(d[:, knn]) & (d[:, knn] <= np.float32(cutoff))
                assert not tie.any(), f"case {i}, params {j}: {int(tie.sum())} points tie at the knn-th distance"
            post = knn_mod.KNN({"knn": knn, "search": search, "sigma": sigma, "cutoff": cutoff}, NCLASSES)
            with torch.no_grad():
                got = post(torch.from_numpy(scan.proj_range.copy()), torch.from_numpy(depth.copy()), torch.from_numpy(argmax.astype(np.int64)),
                           torch.from_numpy(px.astype(np.int64)), torch.from_numpy(py.astype(np.int64))).numpy()
            out[f"c{i}_knn{j}"] = got.astype(np.uint8)
            ours = R.knn_labels_host(scan.proj_range, depth, argmax, px, py, knn, search, sigma, cutoff, NCLASSES)
            print(f"case {i} ({pts.shape[0]} points, {H} x {W}), knn {knn} search {search} sigma {sigma} cutoff {cutoff}: "
                  f"{float((got != plain).mean()):.1%} of the points change label; knn_labels_host differs at "
                  f"{int((ours != got).sum())}")
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
