"""What the BEV-training tests share (tests/test_bev_training_host.py, tests/test_bev_training_gpu.py): the five-beam steep sensor,
grids and per-cell bounds of tests/test_lidar_exact.py's splat tests (imported, not copied: the bounds are those), an input that
reaches every class of pixel the backward treats differently, and an 8-beam sensor for the trainer tests.

The input (2, 2, 37, 5): image 0 is splat_input's dense image with one pixel in ten re-encoded from a NEGATIVE range; image 1 is all but
empty -- every pixel far outside the volume or negative -- so that its grid keeps empty cells, and carries two planted pixels:
  P0  a range value, found by stepping through neighbouring fp32 numbers with the host statement, whose x (or y) grid coordinate is an
      integer in fp32: remainder 0, so its dx = 1 (dy = 1) votes have weight 0 -- into cells that (the image being sparse) nothing else reaches (checked while planting);
  P1  that coordinate 2e-5 above an integer: those votes leave 0 < d < 1e-4 in such cells (below the clamp of the feature plane).
In inverse mode no value decodes to a negative range (1 / max(v, 1e-4) > 0): those pixels fall under the 1e-4 clamp, decode to
10 km and are dropped."""
import functools

import numpy as np
import torch

from tests.test_lidar_exact import (F, MODES, SPLAT_B, SPLAT_GRIDS, SPLAT_IDS, SPLAT_W, U, _Sensor, encode, mode_kw,  # noqa: F401
                                    oracle_of, splat_bounds, splat_input, splat_reference, splat_sensor)

MIN_WEIGHT = float(np.float32(1e-4))


def bev_sensor(grid, pc_range, mode, normalize=True):
    return splat_sensor(grid, pc_range, mode, normalize)


def _geometry(t, img):
    return t._bev_geometry(torch.from_numpy(np.array(img, F)), tables="library")


def _tables(t):
    incl = t.incl.astype(np.float64)
    W = t.width
    a = (F(W) - F(0.5)) - np.arange(W).astype(F)
    a = ((a / F(W)) * F(2)) * F(np.pi) - F(np.pi)
    return np.cos(incl), np.cos(a.astype(np.float64)), np.sin(a.astype(np.float64))


def _plant(t, img, b, mode, above, columns, keep=None):
    """Write into img[b] a pixel whose x or y grid coordinate is an integer in fp32 (above = 0: the range value is searched among the
    300 fp32 numbers on either side of the fp64 solution) or `above` over one, and which then casts the votes it is planted for (keep: a pixel whose weight-0 votes must stay alone in their
    cells); -> (w, h)."""
    gz, gy, gx = t.grid_sizes
    ci, ca, sa = _tables(t)
    for w in columns:
        for h in (2, 1, 3):
            for axis, g, half, trig in ((0, gx, (t.pc_range[3] - t.pc_range[0]) / 2, ca[w]), (1, gy, (t.pc_range[4] - t.pc_range[1]) / 2, sa[w])):
                for k in range(1, g - 1):
                    r = ((2.0 * (k + above) / (g - 1) - 1.0) * half) / (ci[h] * trig)
                    if not 0.5 < r < 25.0:
                        continue
                    v0 = encode(r, mode).reshape(1)
                    steps = np.arange(-300, 301, dtype=np.int32) if above == 0 else np.zeros(1, np.int32)
                    cands = (v0.view(np.int32) + steps).view(F)
                    batch = np.repeat(img[b:b + 1], len(cands), 0)
                    batch[:, 0, w, h] = cands
                    geo = _geometry(t, batch)
                    rem = geo["rem"][axis][:, w, h].numpy()
                    inside = geo["touch"][:, w, h].numpy() & (geo["cell"][axis][:, w, h].numpy() == k)
                    hit = inside & ((rem == 0) if above == 0 else ((rem > 0) & (rem < 1e-4)))
                    if hit.any():
                        old = img[b, 0, w, h]
                        img[b, 0, w, h] = cands[int(np.argmax(hit))]
                        c = pixel_classes(t, img[b:b + 1])
                        if c["zero_vote" if above == 0 else "low_vote"][0, w, h] and (keep is None or c["zero_vote"][0][keep]):
                            return w, h
                        img[b, 0, w, h] = old
    raise AssertionError("no plantable pixel")


@functools.lru_cache(maxsize=None)
def _bev_input(gi, mode):
    grid, pc_range = SPLAT_GRIDS[gi]
    t = bev_sensor(grid, pc_range, mode)
    img = splat_input(mode).copy()
    rng = np.random.default_rng(77 + gi)
    shape = img[0, 0].shape
    neg = encode(rng.uniform(-0.9, -0.1, shape), mode)
    img[0, 0] = np.where(rng.random(shape) < 0.1, neg, img[0, 0])
    u = rng.random(shape)
    sparse = np.where(u < 0.7, encode(rng.uniform(30.0, 60.0, shape), mode), encode(rng.uniform(-0.9, -0.1, shape), mode))
    img[1, 0] = sparse.astype(F)
    p0 = _plant(t, img, 1, mode, 0.0, range(1, 18))
    p1 = _plant(t, img, 1, mode, 2e-5, range(19, 36), keep=p0)
    img.setflags(write=False)
    return img, p0, p1


def bev_input(grid, pc_range, mode):
    """-> (image (2, 2, 37, 5) fp32, read-only; P0 (w, h); P1 (w, h)), see the module docstring."""
    return _bev_input(SPLAT_GRIDS.index((grid, pc_range)), mode)


def pixel_classes(t, img, points=None):
    """With the host statement alone (fp32, the library's tables; points: the device's own, if given): which pixels were replaced
    (negative decoded range), dropped (cannot touch the volume), cast an in-grid vote of weight 0 into a cell with d = 0, or an
    in-grid vote into a cell with 0 < d < 1e-4; and d, S of the fp32 host splat."""
    x = torch.from_numpy(np.array(img, F))
    geo = t._bev_geometry(x, points, tables="library")
    _, d, S = t.to_voxel_host(x, return_raw=True, tables="library")
    B = x.shape[0]
    dflat = d.reshape(B, -1)
    zero_vote = torch.zeros_like(geo["touch"])
    low_vote = torch.zeros_like(geo["touch"])
    for _, _, _, idx, ok, wx, wy, wz in t._bev_votes(geo):
        dc = torch.gather(dflat, 1, idx.reshape(B, -1)).reshape(idx.shape)
        zero_vote |= ok & (wx * wy * wz == 0) & (dc == 0)
        low_vote |= ok & (dc > 0) & (dc < MIN_WEIGHT)
    return dict(replaced=geo["replaced"].numpy(), dropped=(~geo["touch"]).numpy(), zero_vote=zero_vote.numpy(), low_vote=low_vote.numpy(),
                d=d.numpy(), S=S.numpy())


def upstream(shape, seed=5):
    """A seeded upstream gradient for a volume of `shape`."""
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the trainer tests' sensor: 8 beams, for SMALL's 32 x 8 images --------------------------------------------------------------------
class Eight(_Sensor):
    INCL = (0.05, 0.02, -0.01, -0.04, -0.08, -0.13, -0.2, -0.3)
    HEIGHT = (0.2, 0.2, 0.19, 0.19, 0.18, 0.15, 0.12, 0.11)


TRAIN_GRID, TRAIN_RANGE = [1, 32, 32], [-16., -16., -3., 16., 16., 1.]


def train_sensor():
    return Eight(width=32, grid_sizes=list(TRAIN_GRID), pc_range=list(TRAIN_RANGE))
