#!/usr/bin/env python3
"""Write tests/golden/bev_voxel.npz: what the reference's `to_voxel` computes, and its autograd gradient, recorded on CPU fp64.

    python tools/make_bev_golden.py --reference /path/to/RangeLDM [--out tests/golden/bev_voxel.npz]

The reference's own code does the computing: `point_cloud_to_range_image_KITTI(width=32, grid_sizes=[1, 16, 16],
pc_range=[-16, -16, -3, 16, 16, 1]).to_voxel` (ldm/kitti360_range_image.py over ldm/dataset.py: to_pc_torch, to_voxel,
_splat_points_to_volumes), imported from REFERENCE/ldm.  ldm/dataset.py imports pytorch_lightning for its data module only; where that
package is missing an empty stand-in module takes its place for the import.  The reference allocates its accumulators with torch's
default dtype, so the run sets the default dtype to float64; the per-beam tables stay the float32 arrays of the reference's class.

The input is one seeded (1, 2, 32, 64) image: ranges mostly inside the 32 m x 32 m volume, some beyond it, some values that decode
to a negative range (replaced by the 100 m fill, in place, which cuts their gradient).  Only arrays are written:

    seed      the numpy seed of image and G
    image     (1, 2, 32, 64) float64
    voxel     (1, 2, 16, 16) float64: to_voxel(image)
    G         (1, 2, 16, 16) float64: a seeded weighting of the volume
    grad      (1, 2, 32, 64) float64: d sum(voxel * G) / d image by torch autograd through the reference's code
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
WIDTH, GRID, PC_RANGE = 32, [1, 16, 16], [-16., -16., -3., 16., 16., 1.]


def load_reference(root):
    """The reference's point_cloud_to_range_image_KITTI, imported from ROOT/ldm."""
    try:
        import pytorch_lightning  # noqa: F401
    except ImportError:
        stub = types.ModuleType("pytorch_lightning")
        stub.LightningDataModule = object
        sys.modules["pytorch_lightning"] = stub
    sys.path.insert(0, os.path.join(root, "ldm"))
    from kitti360_range_image import point_cloud_to_range_image_KITTI
    return point_cloud_to_range_image_KITTI


def make_image(seed=SEED):
    """(1, 2, 32, 64) float64, linear range encoding v = (r - 20) / 40: four pixels in five within 0.5 .. 22 m, one in ten at 30 .. 60 m,
    one in ten with a value below -0.5 (a negative decoded range); remission uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    shape = (1, WIDTH, 64)
    u = rng.random(shape)
    metres = np.where(u < 0.8, rng.uniform(0.5, 22.0, shape), np.where(u < 0.9, rng.uniform(30.0, 60.0, shape), rng.uniform(-30.0, -1.0, shape)))
    image = np.stack([(metres - 20.0) / 40.0, rng.uniform(0, 1, shape)], 1)
    G = rng.standard_normal((1, 2 * GRID[0], GRID[1], GRID[2]))
    return image, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bev_voxel.npz"))
    a = ap.parse_args()
    Sensor = load_reference(a.reference)
    torch.set_default_dtype(torch.float64)
    t = Sensor(width=WIDTH, grid_sizes=list(GRID), pc_range=list(PC_RANGE))
    image, G = make_image()
    x = torch.from_numpy(image).requires_grad_()
    voxel = t.to_voxel(x)
    (grad,) = torch.autograd.grad((voxel * torch.from_numpy(G)).sum(), x)
    assert voxel.dtype == torch.float64 and tuple(voxel.shape) == G.shape
    np.savez_compressed(a.out, seed=np.int64(SEED), image=image, voxel=voxel.detach().numpy(), G=G, grad=grad.numpy())
    occupied = int((voxel[:, 0] > 0).sum())
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; {occupied} of {GRID[1] * GRID[2]} cells occupied, "
          f"{int((x[:, 0] * 40 + 20 < 0).sum())} pixels decode negative, |grad| max {float(grad.abs().max()):.3g}")


if __name__ == "__main__":
    main()
