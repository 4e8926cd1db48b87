"""Synthetic sweeps of a sensor with known per-beam tables, the grids and the gates of the Hough tests (test_hough_host.py,
test_hough_gpu.py): what sensor.estimate_sensor must recover."""
import numpy as np

from rangeldm_amd.range_image import _KITTI_HEIGHT, _KITTI_ZENITH
from rangeldm_amd.sensor import HoughGrid

KITTI_INCL = -np.array(_KITTI_ZENITH, np.float32).astype(np.float64)        # the tables the shipped class hands the library
KITTI_HEIGHT = np.array(_KITTI_HEIGHT, np.float32).astype(np.float64)
# 16 beams in two height groups (as the KITTI-360 sensor's two laser blocks), top beam first
TWO_GROUP_INCL = np.linspace(-0.0302, 0.4187, 16)
TWO_GROUP_HEIGHT = np.concatenate([0.21 - 0.0015 * np.arange(8), 0.125 - 0.0012 * np.arange(8)])

# theta from -0.06 in 1 040 rows of 0.5 mrad, h from 0 in 320 bins of 1 mm
GRID = HoughGrid(-0.06, 5e-4, 1040, 0.0, 1e-3, 320)
MIN_SEPARATION = 4
# gates: Hough stage within 1 row and 2 bins of the truth; refined stage per fixture
HOUGH_GATE = (1.0 * GRID.theta_step, 2.0 * GRID.h_step)
KITTI_REFINED_GATE = (1e-6, 1e-5)                                            # rad, m: no jitter
JITTER_REFINED_GATE = (0.25 * GRID.theta_step, 1.0 * GRID.h_step)            # jitter 2e-4 rad
JITTER = 2e-4


def synth_sweep(incl, height, W, seed, jitter=0.0, drop=0.2):
    """One sweep (n, 3) fp32 of the sensor (incl, height): per pixel a range exp(uniform(log 2.5, log 80)), the azimuth of
    to_pc_torch's column centre plus uniform(-0.4, 0.4) of a column, z = height - r sin(incl), xy = r cos(incl); `drop` of the
    returns removed, the rows shuffled.  jitter: sigma [rad] of a Gaussian error of the inclination, per return."""
    rng = np.random.default_rng(seed)
    incl, height = np.asarray(incl, np.float64), np.asarray(height, np.float64)
    H = len(incl)
    r = np.exp(rng.uniform(np.log(2.5), np.log(80.0), (W, H)))
    azi = (W - 0.5 - np.arange(W)) / W * 2.0 * np.pi - np.pi
    azi = azi[:, None] + rng.uniform(-0.4, 0.4, (W, H)) * (2.0 * np.pi / W)
    inc = np.broadcast_to(incl[None, :], (W, H))
    if jitter:
        inc = inc + jitter * rng.standard_normal((W, H))
    z = height[None, :] - r * np.sin(inc)
    xy = r * np.cos(inc)
    pts = np.stack([xy * np.cos(azi), xy * np.sin(azi), z], -1)[rng.uniform(size=(W, H)) >= drop]
    return pts[rng.permutation(len(pts))].astype(np.float32)


def kitti_sweeps():
    """Recovery of the shipped KITTI-360 tables: two sweeps, W = 1024, no jitter."""
    return [synth_sweep(KITTI_INCL, KITTI_HEIGHT, 1024, seed) for seed in (0, 1)]


def jitter_sweeps():
    """16 beams in two height groups, four sweeps, W = 256, jitter 2e-4 rad."""
    return [synth_sweep(TWO_GROUP_INCL, TWO_GROUP_HEIGHT, 256, seed, jitter=JITTER) for seed in (0, 1, 2, 3)]


def worst(tables, incl, height):
    """(largest |incl error| [rad], largest |height error| [m]) of SensorTables against the truth."""
    return float(np.abs(tables.incl - incl).max()), float(np.abs(tables.height - height).max())
