"""python -m rangeldm_amd.calibrate_sensor CLOUD_DIR --beams 64 --out sensor.json

Estimates a sensor's per-beam tables (mounting height, inclination) from a folder of its sweeps by Hough voting
(rangeldm_amd/sensor.py, csrc/hough.hip) and writes them as JSON: what range_image.point_cloud_to_range_image_tables (and
through it project, to_pc_torch, to_voxel and the trainers) needs for a sensor the project ships no constants for.

CLOUD_DIR holds `.bin` sweeps (float32, --columns per point: x y z remission ...) and / or `.npy` arrays (n, >= 3), taken in
sorted order.  Prints one JSON object:

    height, incl     the tables, top beam first (incl [rad] positive downwards, height [m])
    votes, support   per beam: its Hough peak, and the returns its line was fitted to
    points           valid returns that voted
    fill             the share of pixels `project` fills, averaged over up to 16 of the clouds:
                     fill.estimated with the estimated tables, fill.spherical with uniform inclinations (linspace between the
                     extreme estimated ones) and zero heights -- the projection the RangeLDM paper argues against.
                     The estimated tables should fill clearly more.

--out writes the tables alone (SensorTables.save), --json the printed object.
"""
import argparse
import glob
import json
import os

import numpy as np
import torch

from . import sensor as S

FILL_CLOUDS = 16


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m rangeldm_amd.calibrate_sensor",
                                 description="per-beam height / inclination tables of a LiDAR from its sweeps, by Hough voting")
    ap.add_argument("cloud_dir")
    ap.add_argument("--beams", type=int, required=True, help="lasers of the sensor")
    ap.add_argument("--out", default=None, help="write the tables (SensorTables JSON) here")
    ap.add_argument("--limit", type=int, default=None, help="use the first N files (sorted by name)")
    ap.add_argument("--columns", type=int, default=4, help="float32 columns per point in the .bin files")
    d = S.HoughGrid.default()
    ap.add_argument("--theta-min", type=float, default=d.theta_min, help="lowest inclination of the grid [rad]")
    ap.add_argument("--theta-step", type=float, default=d.theta_step)
    ap.add_argument("--n-theta", type=int, default=d.n_theta)
    ap.add_argument("--h-min", type=float, default=d.h_min, help="lowest height of the grid [m]")
    ap.add_argument("--h-step", type=float, default=d.h_step)
    ap.add_argument("--n-h", type=int, default=d.n_h, help="height bins, at most 4096")
    ap.add_argument("--d-min", type=float, default=d.d_min, help="returns closer than this in the ground plane take no part [m]")
    ap.add_argument("--d-max", type=float, default=d.d_max)
    ap.add_argument("--min-separation", type=int, default=None, help="rows suppressed either side of a picked beam (4)")
    ap.add_argument("--no-refine", action="store_true", help="stop at the Hough stage's bin centres")
    ap.add_argument("--width", type=int, default=1024, help="azimuth bins of the range image `fill` is measured on")
    ap.add_argument("--json", default=None, help="also write the result object to this file")
    return ap


def load_cloud(path, columns=4):
    """(n, >= 3) fp32 array of a `.bin` (np.fromfile(float32).reshape(-1, columns)) or `.npy` sweep."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError(f"{path}: expected an (n, >= 3) array, got {a.shape}")
        return np.ascontiguousarray(a, np.float32)
    return np.fromfile(path, dtype=np.float32).reshape(-1, columns)


def fill_share(sensor, clouds, device):
    """Mean share of pixels sensor.project fills (mask) over the clouds; a cloud without a remission column gets zeros."""
    shares = []
    for c in clouds:
        pc = torch.from_numpy(c).to(device)
        if pc.shape[1] < 4:
            pc = torch.cat([pc[:, :3], torch.zeros((pc.shape[0], 1), device=device)], 1)
        shares.append(float(sensor.project(pc)["mask"].float().mean()))
    return sum(shares) / len(shares)


def main(argv=None):
    from .range_image import point_cloud_to_range_image_tables
    a = build_parser().parse_args(argv)
    files = sorted(glob.glob(os.path.join(a.cloud_dir, "*.bin")) + glob.glob(os.path.join(a.cloud_dir, "*.npy")))[:a.limit]
    if not files:
        raise FileNotFoundError(f"{a.cloud_dir}: no .bin or .npy clouds")
    grid = S.HoughGrid(a.theta_min, a.theta_step, a.n_theta, a.h_min, a.h_step, a.n_h, a.d_min, a.d_max)
    device = torch.device("cuda")
    acc = S.HoughAccumulator(grid, device)
    for f in files:                                          # one sweep on the device at a time
        acc.add([load_cloud(f, a.columns)])
    mx, arg = acc.row_peaks()
    clouds = (load_cloud(f, a.columns) for f in files)       # a second pass over the files for the fit

    def refine(c, incl, height, tol, d_min, d_max):
        return S.refine_beams(c, incl, height, tol, d_min=d_min, d_max=d_max, device=device)
    tables = S.tables_from_peaks((mx.cpu().numpy(), arg.cpu().numpy()), refine, clouds, a.beams, grid, a.min_separation,
                                 not a.no_refine, None)
    if a.out:
        tables.save(a.out)
    some = [load_cloud(f, a.columns) for f in files[:FILL_CLOUDS]]
    spherical = point_cloud_to_range_image_tables(np.zeros(a.beams), np.linspace(tables.incl.min(), tables.incl.max(), a.beams),
                                                  width=a.width)
    fill = {"estimated": fill_share(point_cloud_to_range_image_tables(tables, width=a.width), some, device),
            "spherical": fill_share(spherical, some, device)}
    result = {**tables.to_dict(), "points": acc.points, "fill": fill, "files": len(files)}
    text = json.dumps(result, sort_keys=True)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    return result


if __name__ == "__main__":
    main()
