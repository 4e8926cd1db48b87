"""lidar.hip at small, odd shapes: every kernel against a plain statement of the same operation, bit for bit wherever the
operation is a fixed sequence of single fp32 roundings, and within a derived bound where the summation order is free.

tests/test_lidar.py runs the kernels at the sensors' own shapes (H = 64 / 32, W = 1024).  Here the sensors are test-only
subclasses with 5, 3 and 1 beams, W is odd or no multiple of any tile, and the inputs are planted so that each branch and
each wrap-around of the index arithmetic decides at least one output value.

  a. range image -> points    numpy fp32 restatement of range_to_points_kernel, one rounding per operation: bit-exact in
                              linear and inverse mode; 2e-5 in log mode (exp2f is the device's libm)
  b. ordered depth filter     `pc[norm < d]` in numpy fp32 with the kernel's operation order: bit-exact
  c. 8-bit rendering          `(clip(x, 0, 1) * float32(255)).astype(uint8)`: bit-exact, every channel
  d. projection               returns aimed at pixel centres, so that an ulp of atan2f cannot move one (asserted on the CPU
                              with the oracle alone): remission and both masks bit-exact in every mode, range bit-exact in
                              linear and inverse mode, 1e-6 in log mode (log2f)
  e. BEV splat                cell by cell against the fp64 accumulation of the same fp32 votes, within the rounding bound
                              of a k-term fp32 sum in any order (derived in test_hip_splat_cell_by_cell)
"""
import functools

import numpy as np
import pytest
import torch

from oracle.lidar import LidarOracle
from rangeldm_amd import range_image as RI

F = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32
MODES = ("linear", "log", "inverse")


def mode_kw(mode):
    return {"log": mode == "log", "inverse": mode == "inverse"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    """fp32 array -> its bit patterns (array_equal on floats would take -0.0 for 0.0)."""
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- test-only sensors -------------------------------------------------------------------------------------------
class _Sensor(RI.point_cloud_to_range_image):
    """Tables from the subclass; get_row_inds -> None: the device searches the nearest beam (like KITTI-360)."""
    INCL, HEIGHT = (), ()

    def __init__(self, **kw):
        self.height = np.array(self.HEIGHT, dtype=F)
        self.incl = np.array(self.INCL, dtype=F)
        self.zenith = -self.incl
        self.H = len(self.HEIGHT)
        super().__init__(**kw)

    def get_row_inds(self, pc):
        return None


class _Rows:
    """Explicit rows from column 4 and min_depth = 2.0 (like nuScenes)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.min_depth = 2.0

    def get_row_inds(self, pc):
        return pc[:, 4].to(torch.int32)


class Five(_Sensor):
    INCL, HEIGHT = (0.03, -0.02, -0.1, -0.2, -0.35), (0.2, 0.19, 0.18, 0.12, 0.11)


class Three(_Sensor):                 # h - 2 = h + 1 (mod 3)
    INCL, HEIGHT = (0.03, -0.1, -0.3), (0.2, 0.15, 0.1)


class One(_Sensor):
    INCL, HEIGHT = (-0.05,), (0.15,)


class FiveSteep(_Sensor):             # beams that leave a 4 m high volume through its floor and its ceiling within 10 m
    INCL, HEIGHT = (0.5, 0.2, -0.02, -0.2, -0.45), (0.2, 0.19, 0.18, 0.12, 0.11)


class FiveRows(_Rows, Five):
    pass


class ThreeRows(_Rows, Three):
    pass


class OneRows(_Rows, One):
    pass


def oracle_of(t):
    return LidarOracle(t.incl, t.height, width=t.width, grid_sizes=t.grid_sizes, pc_range=t.pc_range, log=t.log,
                       inverse=t.inverse, normalize_volume_densities=t.normalize_volume_densities)


# ---- a. range image -> points --------------------------------------------------------------------------------------
def to_pc_fp32(img, incl, height, mode):
    """range_to_points_kernel in numpy fp32: every operation is one fp32 rounding, in the kernel's order.  Tables as the
    host code builds them: cos / sin in fp64 of the fp32 angle, rounded once; the azimuth in fp32 steps."""
    img = np.asarray(img, F)
    B, C, W, H = img.shape
    incl, height = np.asarray(incl, F), np.asarray(height, F)
    cos_incl, sin_incl = np.cos(incl.astype(np.float64)).astype(F), np.sin(incl.astype(np.float64)).astype(F)
    a = (F(W) - F(0.5)) - np.arange(W).astype(F)
    a = a / F(W)
    a = a * F(2)
    a = a * F(np.pi)
    a = a - F(np.pi)
    cos_azi, sin_azi = np.cos(a.astype(np.float64)).astype(F), np.sin(a.astype(np.float64)).astype(F)
    v = img[:, 0]
    if mode == "log":                 # exp2 in fp64, rounded once: the device's exp2f is within its libm's ulp of this
        r = np.exp2((v * F(6)).astype(np.float64)).astype(F) - F(1)
    elif mode == "inverse":
        r = F(1) / np.maximum(v, F(0.0001))
    else:
        r = v * F(40) + F(20)
    r = np.where(r < 0, F(100), r).astype(F)
    xy = r * cos_incl[None, None, :]
    z = height[None, None, :] - r * sin_incl[None, None, :]
    x = xy * cos_azi[None, :, None]
    y = xy * sin_azi[None, :, None]
    cols = [x.reshape(B, -1), y.reshape(B, -1), z.reshape(B, -1)]
    if C > 1:
        cols.append(img[:, 1].reshape(B, -1))
    out = np.stack(cols, 2)
    assert out.dtype == F
    return out


TO_PC_SHAPES = [(Five, (2, 2, 37, 5)), (One, (1, 1, 1, 1)), (Three, (3, 2, 65, 3)), (Five, (2, 3, 129, 5))]


def to_pc_input(shape, mode, seed=3):
    """Encoded ranges over the whole decodable span plus, planted at the front of every image: values that decode to a
    negative range (-> fill 100), to exactly 0, -0.0, and (inverse mode) values at and below the max(v, 1e-4) clamp."""
    rng = np.random.default_rng(seed)
    B, C, W, H = shape
    if mode == "linear":
        x = rng.uniform(-0.7, 2.2, (B, W, H))
        special = [-0.5, -0.6, -0.0, 0.0, -0.5000001, 2.0, -100.0]                 # -0.5 * 40 + 20 = 0 exactly
    elif mode == "log":
        x = rng.uniform(-0.2, 1.1, (B, W, H))                                       # up to 2^6.6 - 1 = 96 m
        special = [0.0, -0.0, -0.1, -1e-8, 1.0, 0.5]
    else:
        x = rng.uniform(0.008, 1.5, (B, W, H))
        special = [0.0001, 0.00009, 0.0, -0.0, -3.0, 0.00010001, 1.0, float("inf")]
    x = x.astype(F)
    flat = x.reshape(B, -1)
    k = min(len(special), flat.shape[1])
    flat[:, :k] = np.array(special[:k], F)
    if flat.shape[1] > 2 * k:
        flat[:, -k:] = np.array(special[:k], F)[::-1]
    img = np.zeros(shape, F)
    img[:, 0] = flat.reshape(B, W, H)
    img[:, 1:] = rng.uniform(-1, 2, (B, C - 1, W, H)).astype(F)
    return img


@pytest.mark.parametrize("mode", MODES)
def test_to_pc_restatement_matches_oracle_and_golden(golden, mode):
    """The fp32 restatement that the device is held to bit for bit is itself the reference's to_pc_torch within 2e-5 (the
    oracle takes cos / sin in fp32, the host code rounds the fp64 values: an ulp of the table, 2e-7 relative, which passes
    2e-5 only beyond the 100 m the project's tolerance was set for; the 1e-4 clamp of the inverse mode decodes to 10 km)."""
    g = golden("lidar")
    tag = {"linear": "kitti", "log": "kittilog", "inverse": "kittiinv"}[mode]
    t = RI.point_cloud_to_range_image_KITTI(**mode_kw(mode))
    assert np.abs(to_pc_fp32(g[f"lidar_{tag}_img"], t.incl, t.height, mode) - g[f"lidar_{tag}_pc_ref"]).max() < 2e-5
    for cls, shape in TO_PC_SHAPES:
        s = cls(**mode_kw(mode))
        img = to_pc_input(shape, mode)
        want = oracle_of(s).to_pc(img)
        got = to_pc_fp32(img, s.incl, s.height, mode)
        assert got.shape == want.shape == (shape[0], shape[2] * shape[3], 4 if shape[1] > 1 else 3)
        tol = np.maximum(2e-5, 2e-7 * np.abs(want))
        assert (np.abs(got - want) <= tol).all()


def test_to_pc_input_reaches_every_decode_branch():
    for shape in (s for _, s in TO_PC_SHAPES if s[2] > 1):
        lin = to_pc_input(shape, "linear")[:, 0]
        r = lin * F(40) + F(20)
        assert (r < 0).any() and (r == 0).any() and (r > 100).any()
        inv = to_pc_input(shape, "inverse")[:, 0]
        assert (inv < F(0.0001)).any() and (inv == F(0.0001)).any() and (inv > F(0.0001)).any()
        lg = to_pc_input(shape, "log")[:, 0]
        assert (lg < 0).any() and (lg == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls,shape", TO_PC_SHAPES, ids=lambda v: getattr(v, "__name__", None) or "x".join(map(str, v)))
def test_hip_to_pc_bit_exact(cls, shape, mode):
    t = cls(**mode_kw(mode))
    img = to_pc_input(shape, mode)
    want = to_pc_fp32(img, t.incl, t.height, mode)
    got = t.to_pc_torch(dev(img)).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(bits(got[..., 3:]), bits(want[..., 3:]))                  # remission: copied bits
    if mode == "log":
        assert (np.abs(got - want) < 2e-5).all()
    else:
        assert np.array_equal(bits(got), bits(want))
    # one channel gives xyz only, equal to the first three columns of the two-channel result; later channels are not read
    xyz = t.to_pc_torch(dev(img[:, :1])).cpu().numpy()
    assert xyz.shape == (shape[0], shape[2] * shape[3], 3)
    if shape[1] > 1:
        assert np.array_equal(bits(xyz), bits(got[..., :3]))
    if shape[1] > 2:
        assert np.array_equal(bits(t.to_pc_torch(dev(img[:, :2])).cpu().numpy()), bits(got))


# ---- b. ordered depth filter ----------------------------------------------------------------------------------------
MAX_DEPTH = 40.0
FILTER_N = (1, 255, 256, 257, 1000, 65809)          # 65 809 = 257 * 256 + 17: chunk 257 runs the prefix loop twice
PATTERNS = ("all", "none", "last", "seventh", "mixed")


def keep_fp32(pc, max_depth):
    """keep_point in numpy fp32: ((x*x + y*y) + z*z), sqrt, strict comparison."""
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
    d2 = (x * x + y * y) + z * z
    assert d2.dtype == F
    return np.sqrt(d2) < F(max_depth)


def filter_cloud(N, cols, pattern, seed):
    """(N, cols) fp32.  Dropped points alternate between far ones and points at exactly max_depth: (3, 4, 0) * 8 and its
    permutations have the exact norm 40.  `mixed` scatters points within a few ulp of the boundary: there the fp32
    statement decides."""
    rng = np.random.default_rng(seed)
    inside = rng.uniform(-20, 20, (N, cols)).astype(F)                            # |xyz| <= 34.7
    far = rng.uniform(30, 60, (N, cols)).astype(F)                                # |xyz| >= 51.9
    edge = np.array([[24, 32, 0], [0, -24, 32], [-32, 0, 24], [24, 0, -32]], F)[rng.integers(0, 4, N)]
    outside = far.copy()
    outside[::2, :3] = edge[::2]
    i = np.arange(N)
    keep = {"all": i >= 0, "none": i < 0, "last": i == N - 1, "seventh": i % 7 == 0, "mixed": rng.random(N) < 0.5}[pattern]
    pc = np.where(keep[:, None], inside, outside)
    if pattern == "mixed":
        near = edge * (F(1) + rng.integers(-3, 4, (N, 1)).astype(F) * F(2.0 ** -23))
        pc[1::3, :3] = near[1::3]
    if cols == 4:
        pc[:, 3] = rng.uniform(0, 1, N).astype(F)
    return pc.astype(F), keep


def test_filter_patterns_are_what_they_say():
    """The fp32 statement keeps exactly the planted pattern, drops points at exactly max_depth, and `mixed` has points on
    both sides within a few ulp of it."""
    for cols in (3, 4):
        for p in PATTERNS[:4]:
            pc, keep = filter_cloud(1000, cols, p, 5)
            assert np.array_equal(keep_fp32(pc, MAX_DEPTH), keep)
            assert np.array_equal(LidarOracle.filter_points(pc, MAX_DEPTH), pc[keep])
        pc, _ = filter_cloud(1000, cols, "none", 5)
        on = np.sqrt((pc[:, :3].astype(np.float64) ** 2).sum(1)) == MAX_DEPTH
        assert on.sum() >= 400
        pc, _ = filter_cloud(1000, cols, "mixed", 5)
        k = keep_fp32(pc, MAX_DEPTH)
        near = np.abs(np.sqrt((pc[:, :3].astype(np.float64) ** 2).sum(1)) - MAX_DEPTH) < 1e-4
        assert (k & near).sum() >= 50 and (~k & near).sum() >= 50
        assert np.array_equal(LidarOracle.filter_points(pc, MAX_DEPTH), pc[k])


@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("cols", (3, 4))
@pytest.mark.parametrize("N", FILTER_N)
def test_hip_filter_bit_exact(N, cols, B):
    t = One()
    rounds = [(p,) for p in PATTERNS] if B == 1 else [("all", "none", "last"), ("seventh", "last", "mixed"),
                                                      ("none", "mixed", "all"), ("last", "seventh", "none")]
    for r, pats in enumerate(rounds):
        pc = np.stack([filter_cloud(N, cols, p, 100 * r + b)[0] for b, p in enumerate(pats)])
        out, counts = t.filter_points(dev(pc), MAX_DEPTH)
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
        assert out.shape == pc.shape and counts.shape == (B,)
        for b in range(B):
            want = pc[b][keep_fp32(pc[b], MAX_DEPTH)]
            assert counts[b] == len(want), (pats, b)
            assert np.array_equal(bits(out[b, :len(want)]), bits(want)), (pats, b)    # rows past counts[b]: unspecified


# ---- c. 8-bit rendering ---------------------------------------------------------------------------------------------
RENDER_SHAPES = [(2, 3, 65, 5), (1, 2, 64, 64), (1, 1, 1, 1), (2, 2, 129, 70)]


def render_input(shape, seed=9):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 1.5, shape).astype(F)
    steps = (np.arange(256) / 255).astype(F)
    special = np.concatenate([steps, np.nextafter(steps[1:], F(0)), np.array([0.0, -0.0, 1.0, -1.0, 2.0, 1e-9, 0.99999994,
                              1.0000001, -1e-9, 3e38, -3e38], F)])
    flat = x.reshape(shape[0], shape[1], -1)
    n = flat.shape[2]
    for b in range(shape[0]):
        for c in range(shape[1]):
            pos = rng.permutation(n)[:len(special)]
            flat[b, c, pos] = np.roll(special, 17 * (b * shape[1] + c))[:len(pos)]
    return flat.reshape(shape)


def render_ref(x, c):
    return np.transpose((np.clip(x[:, c], F(0), F(1)) * F(255)).astype(np.uint8), (0, 2, 1))     # (B, H, W)


def test_render_statement_is_the_oracles():
    x = render_input(RENDER_SHAPES[3])
    for c in range(2):
        assert np.array_equal(render_ref(x, c)[1], LidarOracle.render_u8(x[1], c))
    assert len(np.unique(render_ref(x, 0))) == 256


@pytest.mark.gpu
@pytest.mark.parametrize("shape", RENDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hip_render_bit_exact(shape):
    x = render_input(shape)
    xd = dev(x)
    for c in range(shape[1]):
        got = RI.render_u8(xd, channel=c)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[3], shape[2])
        assert np.array_equal(got.cpu().numpy(), render_ref(x, c)), c
    with pytest.raises(RuntimeError, match="bad shape"):
        RI.render_u8(xd, channel=shape[1])


# ---- d. projection --------------------------------------------------------------------------------------------------
# (sensor, explicit rows?, W, stride); explicit rows are read from column 4, so they need stride >= 5
PROJ_CASES = [(Five, False, 37, 4), (Five, True, 64, 5), (Five, False, 65, 6), (Five, True, 37, 6), (Five, False, 64, 5),
              (Three, False, 65, 5), (Three, True, 2, 5), (Three, True, 64, 6), (One, False, 1, 4), (One, True, 37, 5),
              (One, False, 2, 6), (One, True, 65, 6)]
ROWS_OF = {Five: FiveRows, Three: ThreeRows, One: OneRows}
PROJ_IDS = [f"{c.__name__}{'Rows' if e else ''}-W{w}-s{s}" for c, e, w, s in PROJ_CASES]
ORIGIN_REMISSION = 0.61


def sensor_for(cls, explicit, W, mode):
    return (ROWS_OF[cls] if explicit else cls)(width=W, **mode_kw(mode))


@functools.lru_cache(maxsize=None)
def scene(cls, explicit, W, stride, special):
    """A sweep for the sensor: (points (n, stride) fp32, intended (n, 2) int (row, col)), in random order.  Row -1: the
    return is dropped; col -2: the return is not aimed, its column is whatever the oracle says.

    Aimed returns sit at the centre of their pixel: azimuth of the column centre, elevation of the beam seen from the beam's
    own height.  Half the pixels are occupied, with 1 to 4 returns each, with exact range ties (same xyz, other remission);
    one pixel in seven holds only returns beyond 100 m, which all clamp to 100 and tie.  For W >= 37 pixel (0, 5) holds three
    returns beyond 100 m and (0, 6) a three-way tie in front of a farther return.

    special=False and W >= 37: two zones are cleared and replanted.
      cols W-6 .. W-1 and 0 .. 3   only (0, 0) holds returns: (0, W-1) is filled from column 0 across the seam, (0, W-2)
                                   stays missing and has a car-window neighbour across the w seam alone
      cols 8 .. 20                 returns at (H-2, 10) and (1, 16) only: car-window neighbours of rows 0 and H-1 across the h
                                   seam alone, and of rows 1 and H-4 through h + 2 without a wrap
    special=True adds the returns that are not aimed: y = -0.0 and y = +0.0 with x < 0 (azimuth -pi and +pi: colf = W - 0.5,
    which rounds half to even and for even W reaches the col == W clamp, and colf = -0.5), the sensor origin (beam search
    only: range 0), explicit rows outside [0, H), and returns at exactly and just above min_depth (explicit rows only)."""
    t = cls()
    H, incl, height = t.H, t.incl.astype(np.float64), t.height.astype(np.float64)
    rng = np.random.default_rng(1000 * H + 10 * W + stride + 7 * special)
    azi = LidarOracle.azimuth(W).astype(np.float64)
    tail = [7.0] * max(stride - 5, 0)
    occ = rng.random((H, W)) < 0.5
    if W >= 37 and not special:
        occ[:, W - 6:] = False
        occ[:, :4] = False
        occ[0, 0] = True
        occ[:, 8:21] = False
        occ[max(H - 2, 0), 10] = True
        occ[min(1, H - 1), 16] = True
    pts, want = [], []

    def aimed(h, w, r, rem):
        return [r * np.cos(incl[h]) * np.cos(azi[w]), r * np.cos(incl[h]) * np.sin(azi[w]), height[h] - r * np.sin(incl[h]),
                rem, float(h)] + tail

    if W >= 37:                                                                     # whatever the draw: both kinds of tie
        occ[0, 5:7] = False
        for j, r in enumerate((101.0, 150.0, 120.0)):
            pts.append(aimed(0, 5, r, 0.2 + 0.1 * j))
        for j, r in enumerate((33.0, 17.5, 17.5, 17.5)):
            pts.append(aimed(0, 6, r, 0.2 + 0.1 * j))
        want += [(0, 5)] * 3 + [(0, 6)] * 4
    for h, w in zip(*np.nonzero(occ)):
        k = int(rng.integers(1, 5))
        if rng.random() < 0.15:
            ranges = rng.choice([101.0, 120.0, 150.0, 100.5], k)
        else:
            ranges = rng.uniform(2.5, 99.0, k)
            if k > 1:
                ranges[1:] = np.where(rng.random(k - 1) < 0.5, ranges[0], ranges[1:])
        for r in ranges:
            pts.append(aimed(h, w, r, rng.uniform(0, 1)))
            want.append((h, w))
    if special:
        h = H // 2
        for y0, col in ((-0.0, min(int(np.round(W - 0.5)), W - 1)), (0.0, 0)):
            p = aimed(h, 0, 2.25, 0.123)
            p[0], p[1] = -2.25 * np.cos(incl[h]), y0
            pts.append(p)
            want.append((h, col))
        if explicit:
            for row in (-1, H, 1000, -7):
                p = aimed(0, W // 2, 2.2, 0.5)
                p[4] = float(row)
                pts.append(p)
                want.append((-1, -2))
            pts.append([0.0, -2.0, 0.0, 0.31, H - 1.0] + tail)                      # exactly min_depth: dropped
            want.append((-1, -2))
            pts.append([0.0, float(np.nextafter(F(-2.0), F(-3.0))), 0.0, 0.32, H - 1.0] + tail)
            want.append((H - 1, -2))
        else:
            pts.append([0.0, 0.0, float(t.height[h]), ORIGIN_REMISSION, float(h)] + tail)
            want.append((h, -2))
    pts = np.array([p[:max(stride, 5)][:stride] for p in pts], F).reshape(-1, stride)
    want = np.array(want, np.int64).reshape(-1, 2)
    perm = rng.permutation(len(pts))
    return pts[perm], want[perm]


def norm_fp32(xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.sqrt((x * x + y * y) + z * z)


def kept_subset(o, pts, explicit):
    """What the kernel keeps: explicit rows inside [0, H) and (min_depth = 2) fp32 norm > 2; the beam search keeps all."""
    if not explicit:
        return pts, o.row_inds_nearest_beam(pts)
    rows = pts[:, 4].astype(np.int32)
    keep = (rows >= 0) & (rows < o.H) & (norm_fp32(pts) > F(2.0))
    return pts[keep], rows[keep]


def oracle_project(o, pts, explicit):
    """(image (2, W, H), mask (W, H), car-window mask (W, H), raw (H, W, 2)) of the reference's pipeline on the kept subset."""
    kept, rows = kept_subset(o, pts, explicit)
    with np.errstate(divide="ignore"):                                             # inverse mode: 1 / 0 at the origin return
        raw = o.project(kept, rows)
    filled, mask, car = o.process_miss_value(raw)
    return np.transpose(o.normalize(filled), (2, 1, 0)), mask.T, car.T, raw


def origin_pixel(o, t):
    hs = t.H // 2
    return hs, int(o.col_inds(np.array([[0, 0, t.height[hs], 0]], F))[0])


@pytest.mark.parametrize("special", (False, True), ids=("zones", "special"))
@pytest.mark.parametrize("cls,explicit,W,stride", PROJ_CASES, ids=PROJ_IDS)
def test_projection_scene_is_decided_by_the_oracle_alone(cls, explicit, W, stride, special):
    """The condition under which exactness may be demanded: every aimed return lands in its intended (row, column) with a
    margin no ulp of atan2 can cross, and the planted content is really there."""
    pts, want = scene(cls, explicit, W, stride, special)
    t = sensor_for(cls, explicit, W, "linear")
    o = oracle_of(t)
    H = o.H
    assert pts.dtype == F and pts.shape[1] == stride
    aimed = want[:, 1] >= 0
    assert np.array_equal(o.col_inds(pts)[aimed], want[aimed, 1])
    frac = o.col_coord(pts)
    off_centre = np.abs(frac - np.round(frac))
    halfway = (pts[:, 1] == 0) & (pts[:, 0] < 0)                                     # azimuth +-pi: .5 exactly, exact in fp32
    assert (off_centre[aimed & ~halfway] < 0.01).all()
    kept, rows = kept_subset(o, pts, explicit)
    if explicit:
        given = pts[:, 4].astype(np.int64)
        dropped = want[:, 0] < 0
        assert np.array_equal(given[~dropped], want[~dropped, 0]) and len(kept) == (~dropped).sum()
    else:
        assert np.array_equal(rows, want[:, 0])
        if H > 1:
            err = np.sort(o.beam_errors(pts), axis=1)
            assert (err[:, 1] - err[:, 0] > 1e-3).all()                             # atan2f's ulp is 1e-7
    img, mask, car, raw = oracle_project(o, pts, explicit)
    # returns per pixel, and pixels whose winner is decided by the index alone
    zz = kept[:, :3].copy()
    zz[:, 2] -= t.height[rows]
    rng_k = np.minimum(np.linalg.norm(zz, axis=1, ord=2), F(100))
    pixels = {}
    for i, key in enumerate(zip(rows.tolist(), o.col_inds(kept).tolist())):
        pixels.setdefault(key, []).append(i)
    tied = [v for v in pixels.values() if (rng_k[v] == rng_k[v].min()).sum() > 1]
    if W >= 37:
        assert sum(len(v) >= 3 for v in pixels.values()) >= 3
        assert sum(rng_k[v].min() < 100 for v in tied) >= 2 and sum(rng_k[v].min() == 100 for v in tied) >= 1
        assert all(len({float(pts_rem) for pts_rem in kept[v, 3]}) == len(v) for v in tied)      # the winner is visible
    if special:
        assert halfway.sum() == 2 and (off_centre[halfway] == 0.5).all() and np.signbit(pts[halfway, 1]).sum() == 1
        assert W % 2 == 1 or np.round(frac[halfway & np.signbit(pts[:, 1])])[0] == W         # even W reaches the clamp
        if explicit:
            given = pts[:, 4].astype(np.int64)
            assert ((given < 0) | (given >= H)).sum() == 4
            d = norm_fp32(pts)
            assert (d == F(2.0)).sum() == 1 and ((d > F(2.0)) & (d < F(2.0001))).sum() == 1
            just = np.flatnonzero((d > F(2.0)) & (d < F(2.0001)))[0]
            jc = o.col_inds(pts[just:just + 1])[0]
            assert raw[H - 1, jc, 1] == pts[just, 3]                                # the nearest of its pixel: visible
        else:                                                                       # the origin return: present, mask false
            hs, c0 = origin_pixel(o, t)
            assert raw[hs, c0, 0] == 0 and raw[hs, c0, 1] == F(ORIGIN_REMISSION) and not mask[c0, hs]
    elif W >= 37:
        present = raw[..., 0] != -1
        assert present[0, 0] and not present[0, W - 6:].any() and mask[W - 1, 0]       # filled from column 0 over the seam
        assert img[1, W - 1, 0] == raw[0, 0, 1]
        after_fill = present | np.roll(present, -1, axis=1)
        still = ~after_fill
        assert still.sum() >= 10 * H                                                # runs of >= 2 missing stay missing
        down, up = np.roll(after_fill, 2, axis=0), np.roll(after_fill, -2, axis=0)
        right, left = np.roll(after_fill, 2, axis=1), np.roll(after_fill, -2, axis=1)
        assert np.array_equal(car.T, still & (down | up | right | left))
        assert (still & left & ~down & ~up & ~right)[:, W - 2:].any()               # only across the w seam, (w + 2) % W
        if H >= 3:
            assert (still & down & ~up & ~right & ~left)[:2].any()                  # only across the h seam, (h - 2) % H
            assert (still & up & ~down & ~right & ~left)[H - 2:].any()              # only across the h seam, (h + 2) % H
        if H >= 5:
            assert (still & up & ~down & ~right & ~left)[:H - 2].any()              # only through h + 2, no wrap
            assert (still & ~car.T).any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls,explicit,W,stride", PROJ_CASES, ids=PROJ_IDS)
def test_hip_projection_bit_exact(cls, explicit, W, stride, mode):
    t = sensor_for(cls, explicit, W, mode)
    o = oracle_of(t)
    for special in (False, True):
        pts, _ = scene(cls, explicit, W, stride, special)
        for order in (slice(None), slice(None, None, -1)):                          # both orders: index ties go the other way
            p = np.ascontiguousarray(pts[order])
            img, mask, car, _ = oracle_project(o, p, explicit)
            x = dev(p)
            before = x.clone()
            got = t.project(x)
            assert torch.equal(x, before)
            jpg = got["jpg"].cpu().numpy()
            assert jpg.shape == (2, W, t.H)
            assert np.array_equal(got["mask"].cpu().numpy(), mask)
            assert np.array_equal(got["car_window_mask"].cpu().numpy(), car)
            assert np.array_equal(bits(jpg[1]), bits(img[1]))
            if mode == "log":
                assert (np.abs(jpg[0] - img[0]) < 1e-6).all()
            else:
                assert np.array_equal(bits(jpg[0]), bits(img[0]))
            if special and not explicit:                                            # the origin return is present ...
                hs, c0 = origin_pixel(o, t)
                assert jpg[1, c0, hs] == F(ORIGIN_REMISSION)
                assert bool(got["mask"][c0, hs]) == (mode == "inverse")             # ... its range is not > 0 (inverse: 1 / 0)


# ---- e. BEV splat ---------------------------------------------------------------------------------------------------
SPLAT_GRIDS = [((3, 7, 5), (-8., -8., -3., 8., 8., 1.)), ((1, 4, 4), (-4., -4., -3., 4., 4., 1.))]
SPLAT_IDS = ["3x7x5", "1x4x4"]
SPLAT_W, SPLAT_B = 37, 2


def encode(metres, mode):
    m = np.asarray(metres, np.float64)
    if mode == "log":
        return (np.log2(m + 1) / 6).astype(F)
    if mode == "inverse":
        return (1 / m).astype(F)
    return ((m - 20) / 40).astype(F)


def splat_input(mode, seed=21):
    """(B, 2, W, 5): four pixels in five within 14 m (inside or just outside the volumes), the rest at 30 .. 60 m."""
    rng = np.random.default_rng(seed)
    shape = (SPLAT_B, SPLAT_W, 5)
    metres = np.where(rng.random(shape) < 0.8, rng.uniform(0.5, 14.0, shape), rng.uniform(30.0, 60.0, shape))
    return np.stack([encode(metres, mode), rng.uniform(0, 1, shape).astype(F)], 1)


def splat_sensor(grid, pc_range, mode, normalize=True):
    return FiveSteep(width=SPLAT_W, grid_sizes=list(grid), pc_range=list(pc_range), normalize_volume_densities=normalize,
                     **mode_kw(mode))


def splat_reference(o, pc):
    """fp64 accumulation of the fp32 votes of `pc` (B, N, 4), and per cell what the error bounds need.  Non-finite points
    cast no vote (the kernel drops them before the float -> int conversion)."""
    pc = np.array(pc, F, copy=True)
    pc[~np.isfinite(pc[:, :, :3]).all(2), :3] = F(1e6)
    idx, w, ok = o.votes(pc)
    ok = ok & (w != 0)
    B = pc.shape[0]
    nvox = int(np.prod(o.grid_sizes))
    k = np.zeros((B, nvox), np.int64)
    sw, swf, swf_abs = (np.zeros((B, nvox), np.float64) for _ in range(3))
    f = np.broadcast_to(pc[:, :, 3:4].astype(np.float64), w.shape)
    for b in range(B):
        m = ok[b]
        np.add.at(k[b], idx[b][m], 1)
        np.add.at(sw[b], idx[b][m], w[b][m].astype(np.float64))
        np.add.at(swf[b], idx[b][m], w[b][m].astype(np.float64) * f[b][m])
        np.add.at(swf_abs[b], idx[b][m], np.abs(w[b][m].astype(np.float64) * f[b][m]))
    shape = (B,) + tuple(o.grid_sizes)
    return {n: v.reshape(shape) for n, v in (("k", k), ("sw", sw), ("swf", swf), ("swf_abs", swf_abs))}


def splat_bounds(ref):
    """Per cell (density bound, feature bound) of a device result against the fp64 planes rounded to fp32; see the docstring
    of test_hip_splat_cell_by_cell."""
    k, sw, swf, A = ref["k"], ref["sw"], ref["swf"], ref["swf_abs"]
    km1 = np.maximum(k - 1, 0)
    gamma = km1 * U / (1 - km1 * U)
    e_d = gamma * sw                                          # device sum against the exact sum
    bound_d = e_d + U * sw                                    # + the rounding of the reference to fp32
    e_n = U * A + gamma * (1 + U) * A
    D = np.maximum(sw, 1e-4)
    e_D = e_d + 1e-4 * U                                      # max() is 1-Lipschitz; float32(1e-4) against 1e-4
    q = np.abs(swf) / D
    bound_f = (e_n / (D - e_D) + np.abs(swf) * e_D / (D * (D - e_D))) * (1 + U) + 2 * U * q
    return e_d, bound_d, bound_f


@pytest.mark.parametrize("grid,pc_range", SPLAT_GRIDS, ids=SPLAT_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_splat_input_reaches_borders_and_crowded_cells(grid, pc_range, mode):
    """With the oracle alone: the input puts votes where the kernel's bounds tests and its atomics matter."""
    t = splat_sensor(grid, pc_range, mode)
    o = oracle_of(t)
    img = splat_input(mode)
    pc = o.to_pc(img)
    gz, gy, gx = grid
    pi = o.grid_coords(pc)
    idx, w, ok = o.votes(pc)
    cast = ok & (w != 0)
    X, Y = idx % gx, (idx // gx) % gy
    border = (X == 0) | (X == gx - 1) | (Y == 0) | (Y == gy - 1)                   # BEV border: x or y
    assert (cast & border).sum() >= 0.25 * cast.sum()
    touches = ((pi > -1) & (pi < np.array([gx, gy, gz], F))).all(2)                 # the kernel's own condition
    for axis, g in ((0, gx), (1, gy), (2, gz)):
        if g == 1:
            assert (pi[..., axis] == 0).all()          # one cell: the coordinate is (..) * 0, no border to cross
            continue
        assert (touches & (pi[..., axis] > -1) & (pi[..., axis] < 0)).any(), axis
        assert (touches & (pi[..., axis] > g - 1) & (pi[..., axis] < g)).any(), axis
    assert (~ok.any(2)).sum() >= 10                                                 # pixels entirely outside
    ref = splat_reference(o, pc)
    assert (ref["k"] >= 8).sum() >= 8
    assert np.allclose(o.to_voxel(img, pc=pc)[:, :gz], np.log1p(ref["sw"]), rtol=1e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid,pc_range", SPLAT_GRIDS, ids=SPLAT_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_hip_splat_cell_by_cell(grid, pc_range, mode, capsys):
    """The device's own to_pc_torch output goes to LidarOracle.to_voxel(img, pc=...), which accumulates in fp64: cells and
    weights are the same fp32 numbers on both sides, and what differs is the order of the fp32 atomic sum and the rounding of
    the products w * f.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, 4.4: a sum of k terms in
    ANY order has error at most gamma_(k-1) sum |x_i|):

      density    d^ = fl-sum of the k votes w_i >= 0 of the cell:    |d^ - d| <= E_d = gamma_(k-1) sum w
                 the reference is d rounded to fp32:                  bound_d = E_d + u d
      feature    numerator n^ = fl-sum of fl(w_i f_i):  each product errs by u |w_i f_i|, the sum by
                 gamma_(k-1) sum |fl(w_i f_i)| <= gamma_(k-1) (1 + u) A,  A = sum |w_i f_i|:   E_n = u A + gamma_(k-1) (1 + u) A
                 denominator D^ = max(d^, float32(1e-4)) against D = max(d, 1e-4):   |D^ - D| <= E_D = E_d + 1e-4 u
                 |n^ / D^ - n / D| <= E_n / D^ + |n| E_D / (D D^),   D^ >= D - E_D
                 one rounding of the quotient (factor 1 + u, and u |q|) and one of the reference (u |q|), q = n / D:
                 bound_f = (E_n / (D - E_D) + |n| E_D / (D (D - E_D))) (1 + u) + 2 u |q|
      log plane  logf(fl(d^ + 1)) against log1p(d): log is 1-Lipschitz on [1, inf), the addition errs by u relative, so the
                 difference is at most E_d + 2 u before logf's own error and the roundings to fp32, for which the project's
                 2e-5 stands:   bound_log = bound_d + 2e-5

    k, sum w, A and n come from the oracle's votes in fp64.  Nothing here is tuned; the largest error / bound is printed."""
    img = splat_input(mode)
    x = dev(img)
    gz = grid[0]
    worst = {}
    for normalize in (False, True):
        t = splat_sensor(grid, pc_range, mode, normalize)
        o = oracle_of(t)
        pc = t.to_pc_torch(x).cpu().numpy()
        got = t.to_voxel(x).cpu().numpy().astype(np.float64)
        assert got.shape == (SPLAT_B, 2 * gz, grid[1], grid[2]) and np.isfinite(got).all()
        want = o.to_voxel(img, pc=pc).astype(np.float64)
        ref = splat_reference(o, pc)
        _, bound_d, bound_f = splat_bounds(ref)
        if not normalize:                                                           # no cell occupied on one side only
            assert np.array_equal(got[:, :gz] != 0, ref["k"] > 0) and np.array_equal(want[:, :gz] != 0, ref["k"] > 0)
        err_d, err_f = np.abs(got[:, :gz] - want[:, :gz]), np.abs(got[:, gz:] - want[:, gz:])
        occ = ref["k"] > 0
        assert (got[:, gz:][~occ] == 0).all()
        if normalize:
            assert (err_d <= bound_d + 2e-5).all()
            worst["log"] = float((err_d[occ] / (bound_d[occ] + 2e-5)).max())
        else:
            assert (err_d <= bound_d).all(), float((err_d[occ] / bound_d[occ]).max())
            worst["density"] = float((err_d[occ] / bound_d[occ]).max())
        assert (err_f <= bound_f).all(), float((err_f[occ] / bound_f[occ]).max())
        worst["feature"] = max(worst.get("feature", 0.0), float((err_f[occ] / bound_f[occ]).max()))
    with capsys.disabled():
        print(f"\nsplat {SPLAT_IDS[SPLAT_GRIDS.index((grid, pc_range))]} {mode}: largest error / bound  " +
              "  ".join(f"{n} {v:.3f}" for n, v in sorted(worst.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("grid,pc_range", SPLAT_GRIDS, ids=SPLAT_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_hip_splat_nonfinite_pixels_and_batch_slots(grid, pc_range, mode):
    """A NaN / +inf / -inf pixel leaves the volume finite and casts no vote unless it decodes to a finite point (-inf decodes
    to the 100 m fill; in inverse mode NaN hits the 1e-4 clamp and +inf decodes to range 0, the beam's origin).  Against the
    oracle the bound is the one derived above; two device results each lie within E (the bound without the reference's
    rounding) of the exact planes, so they agree within 2 E."""
    t = splat_sensor(grid, pc_range, mode, normalize=False)
    o = oracle_of(t)
    gz = grid[0]
    img = splat_input(mode)
    far = encode(3000.0, mode)
    inside = o.votes(o.to_pc(img))[2][0].sum(1)
    n0 = int(np.argmax(inside))                                                     # the pixel with the most votes that count
    assert inside[n0] >= 4
    w0, h0 = divmod(n0, 5)

    def check(image, other=None):
        x = dev(image)
        got = t.to_voxel(x).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        pc = t.to_pc_torch(x).cpu().numpy()
        ref = splat_reference(o, pc)
        want_d, want_f = ref["sw"], ref["swf"] / np.maximum(ref["sw"], 1e-4)
        e_d, bound_d, bound_f = splat_bounds(ref)
        assert np.array_equal(got[:, :gz] != 0, ref["k"] > 0)
        assert (np.abs(got[:, :gz] - want_d) <= bound_d).all() and (np.abs(got[:, gz:] - want_f) <= bound_f).all()
        if other is not None:
            assert (np.abs(got[:, :gz] - other[:, :gz]) <= 2 * e_d).all()
            assert (np.abs(got[:, gz:] - other[:, gz:]) <= 2 * bound_f).all()
        return got, pc

    moved = img.copy()
    moved[0, 0, w0, h0] = far
    vol_moved, pc_moved = check(moved)
    assert not o.votes(pc_moved)[2][0, n0].any()
    for bad in (np.nan, np.inf, -np.inf):
        image = img.copy()
        image[0, 0, w0, h0] = bad
        vol, pc = check(image)
        p = pc[0, n0, :3]
        if not np.isfinite(p).all() or not o.votes(pc)[2][0, n0].any():             # dropped: the volume of the moved image
            check(image, vol_moved)
        else:
            assert mode == "inverse" and bad == np.inf and np.array_equal(p, [0, 0, t.height[h0]])
    # the same image in two batch slots
    twice = np.concatenate([img[:1], img[1:], img[:1]], 0)
    got, _ = check(twice)
    ref = splat_reference(o, t.to_pc_torch(dev(twice)).cpu().numpy())
    e_d, _, bound_f = splat_bounds(ref)
    assert (np.abs(got[0, :gz] - got[2, :gz]) <= 2 * e_d[0]).all()
    assert (np.abs(got[0, gz:] - got[2, gz:]) <= 2 * bound_f[0]).all()
