"""A sensor's per-beam tables -- mounting height and inclination of every laser -- from its own sweeps, by Hough voting
(rangeldm_amd/csrc/hough.hip).  The reference ships two pairs of such tables as constants (ldm/kitti360_range_image.py:19-48,
ldm/nuscenes_range_image.py:20-35); the RangeLDM paper derives them by Hough voting over the dataset, and this module is that
step: what `range_image.point_cloud_to_range_image_tables` needs for a sensor the project has no constants for.

Model.  A return (x, y, z) of beam k satisfies atan2(height[k] - z, d) = incl[k] with d = sqrt(x^2 + y^2)
(ldm/kitti360_range_image.py:51-61, to_pc_torch); incl is positive downwards, incl = -zenith.  With t = tan(incl):

    h = z + d t        a return is a line in the (t, h) plane with slope d; the returns of one beam meet at (t_k, height_k)

Range noise moves a return along its ray, that is along its line: the estimate does not see it.

Stages.  HoughAccumulator votes every return into a (theta, h) grid on the device; pick_beams takes the `beams` strongest rows
(non-maximum suppression along theta) on the host; refine_beams assigns every return to its nearest picked beam in tangent space
and fits z = height - tan(incl) d per beam in closed form, in fp64.  estimate_sensor runs the three and returns SensorTables.

Host statements.  hough_votes_host, row_peaks_host, assign_host restate the kernels in numpy fp32, one correctly rounded
operation per device operation: the device equals them EXACTLY.  moments_host is the fp64 statement of the per-beam sums (the
device adds in another, fixed, order: equal to rounding).  estimate_sensor_host is the whole pipeline over them.  This module
imports neither the oracle nor the reference.
"""
import ctypes as C
import dataclasses
import json
import math

import numpy as np
import torch

from . import _lib

POINT_LIMIT = 1 << 32           # an accumulator's counters are uint32: it takes fewer valid points than this
_CHUNK_POINTS = 1 << 28         # points of one device call (the entry points take fewer than 2^31)


@dataclasses.dataclass(frozen=True)
class HoughGrid:
    """Row i is the inclination theta_min + (i + 1/2) theta_step [rad], bin j the height h_min + (j + 1/2) h_step [m]; returns
    with d = sqrt(x^2 + y^2) outside [d_min, d_max] take no part."""
    theta_min: float
    theta_step: float
    n_theta: int
    h_min: float
    h_step: float
    n_h: int
    d_min: float = 2.0
    d_max: float = 90.0

    def __post_init__(self):
        if not (1 <= int(self.n_theta) <= _lib.RLDM_HOUGH_MAX_THETA and 1 <= int(self.n_h) <= _lib.RLDM_HOUGH_MAX_H):
            raise ValueError(f"n_theta must be in 1 .. {_lib.RLDM_HOUGH_MAX_THETA} and n_h in 1 .. {_lib.RLDM_HOUGH_MAX_H}")
        if not (self.theta_step > 0 and self.h_step > 0 and math.isfinite(self.h_min)):
            raise ValueError("theta_step and h_step must be positive, h_min finite")
        if not (-math.pi / 2 < self.theta_min and self.theta_min + self.n_theta * self.theta_step < math.pi / 2):
            raise ValueError("the inclinations must lie inside (-pi / 2, pi / 2)")
        if not (0 <= self.d_min <= self.d_max < math.inf):
            raise ValueError("0 <= d_min <= d_max < inf")

    @classmethod
    def default(cls):
        """+-0.6 rad in 2 400 rows of 0.5 mrad, +-0.5 m in 1 000 bins of 1 mm: both shipped sensors with room to spare."""
        return cls(-0.6, 5e-4, 2400, -0.5, 1e-3, 1000)

    def theta(self):
        """Row centres, fp64 (n_theta,)."""
        return self.theta_min + (np.arange(self.n_theta, dtype=np.float64) + 0.5) * self.theta_step

    def tan_table(self):
        """float32(tan(float64(theta_i))): the table the device votes with (it has no transcendentals of its own)."""
        return np.tan(self.theta()).astype(np.float32)

    def h_centre(self, j):
        return self.h_min + (np.asarray(j, np.float64) + 0.5) * self.h_step

    def inv_dh(self):
        return np.float32(1.0 / self.h_step)


# ---- host statements ------------------------------------------------------------------------------------------------
def _host_clouds(clouds):
    if torch.is_tensor(clouds) or isinstance(clouds, np.ndarray):
        clouds = [clouds] if clouds.ndim == 2 else list(clouds)
    out = []
    for c in clouds:
        c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        if c.ndim != 2 or c.shape[1] < 3:
            raise ValueError("every cloud must be (n, >= 3)")
        out.append(c)
    return out


def pack_host(clouds, d_min=2.0, d_max=90.0):
    """rldm_hough_pack in numpy: (sum n_i, 2) fp32 pairs (d, z), d = sqrt(x * x + y * y) in fp32, d = -1 where x, y or z is not
    finite or d lies outside [d_min, d_max] (both ends belong).  Order kept."""
    cs = _host_clouds(clouds)
    pts = np.concatenate([c[:, :3].astype(np.float32) for c in cs], 0) if cs else np.zeros((0, 3), np.float32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        d = np.sqrt(x * x + y * y)
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (d >= np.float32(d_min)) & (d <= np.float32(d_max))
    return np.stack([np.where(ok, d, np.float32(-1.0)), z], 1).astype(np.float32)


def hough_votes_host(clouds, grid, packed=None, row_chunk=64):
    """rldm_hough_vote in numpy: uint32 (n_theta, n_h).  Per valid point and row: h = z + d * tan_i; jf = floor((h - h_min) *
    inv_dh); one vote for (i, int(jf)) iff 0 <= jf < n_h -- every step one fp32 operation."""
    p = pack_host(clouds, grid.d_min, grid.d_max) if packed is None else np.asarray(packed, np.float32)
    p = p[p[:, 0] >= 0]
    d, z = p[:, 0][None, :], p[:, 1][None, :]
    tan, h_min, inv_dh, n_h = grid.tan_table(), np.float32(grid.h_min), grid.inv_dh(), int(grid.n_h)
    votes = np.zeros((grid.n_theta, n_h), np.uint32)
    for r0 in range(0, grid.n_theta, row_chunk):
        t = tan[r0:r0 + row_chunk, None]
        with np.errstate(all="ignore"):
            jf = np.floor((z + d * t - h_min) * inv_dh)
            ok = (jf >= 0) & (jf < n_h)
        cell = (np.arange(t.shape[0], dtype=np.int64)[:, None] * n_h + np.where(ok, jf, 0).astype(np.int64))[ok]
        votes[r0:r0 + t.shape[0]] = np.bincount(cell, minlength=t.shape[0] * n_h).reshape(t.shape[0], n_h)
    return votes


def row_peaks_host(votes):
    """rldm_hough_row_max in numpy: per row (largest count, lowest bin attaining it) as int64 arrays; a zero row gives (0, 0)."""
    v = np.asarray(votes)
    return v.max(1).astype(np.int64), v.argmax(1).astype(np.int64)


def candidates(incl, height):
    """(beams, 2) fp32 = (float32(tan(float64(incl_k))), float32(height_k)): what assign compares with."""
    incl, height = np.asarray(incl, np.float64), np.asarray(height, np.float64)
    if incl.ndim != 1 or incl.shape != height.shape or not 1 <= len(incl) <= _lib.RLDM_HOUGH_MAX_BEAMS:
        raise ValueError(f"incl and height must be two vectors of 1 .. {_lib.RLDM_HOUGH_MAX_BEAMS} beams")
    return np.stack([np.tan(incl), height], 1).astype(np.float32)


def _tol(tol):
    t = float(np.float32(tol))
    if not t > 0:
        raise ValueError(f"tol must be positive, got {tol!r}")
    return t


def assign_host(packed, cand, tol):
    """rldm_hough_assign in numpy: int16 (n,).  e_k = |(h_k - z) / d - tan_k| in fp32, the id of the smallest e_k (lowest k on
    ties), -1 for an invalid point or a smallest e_k that is not < float32(tol)."""
    p, c, tol = np.asarray(packed, np.float32), np.asarray(cand, np.float32), np.float32(_tol(tol))
    ids = np.full(len(p), -1, np.int16)
    for i0 in range(0, len(p), 1 << 16):
        d, z = p[i0:i0 + (1 << 16), 0:1], p[i0:i0 + (1 << 16), 1:2]
        with np.errstate(all="ignore"):
            e = np.abs((c[None, :, 1] - z) / d - c[None, :, 0])
        e = np.where(np.isnan(e), np.float32(np.inf), e)
        k = e.argmin(1)
        ok = (d[:, 0] >= 0) & (e[np.arange(len(k)), k] < tol)
        ids[i0:i0 + len(k)] = np.where(ok, k, -1)
    return ids


def moments_host(packed, ids, beams, return_abs=False):
    """rldm_hough_moments in numpy fp64: (counts int64 (beams,), sums fp64 (beams, 4) = sum d, sum z, sum d^2, sum d z) over the
    points assigned to each beam.  return_abs: also the sums of the absolute terms, what a rounding bound scales with."""
    p, ids = np.asarray(packed, np.float32).astype(np.float64), np.asarray(ids)
    counts, sums, mags = np.zeros(beams, np.int64), np.zeros((beams, 4)), np.zeros((beams, 4))
    for k in range(beams):
        d, z = p[ids == k, 0], p[ids == k, 1]
        terms = np.stack([d, z, d * d, d * z], 1)
        counts[k], sums[k], mags[k] = len(d), terms.sum(0), np.abs(terms).sum(0)
    return (counts, sums, mags) if return_abs else (counts, sums)


# ---- host steps shared by both pipelines ----------------------------------------------------------------------------
def pick_beams(row_max, row_arg, beams, min_separation, grid):
    """The `beams` strongest rows of an accumulator: take the row with the largest maximum (the lowest such row on ties), drop
    every row within `min_separation` rows of it, repeat.  ValueError when fewer than `beams` rows with a non-zero maximum
    remain.  -> (incl, height, votes): the bin centres, sorted top beam first (ascending incl, as the shipped tables), and
    their vote counts."""
    m = np.asarray(row_max.cpu() if torch.is_tensor(row_max) else row_max).astype(np.int64).copy()
    a = np.asarray(row_arg.cpu() if torch.is_tensor(row_arg) else row_arg).astype(np.int64)
    beams, sep = int(beams), int(min_separation)
    if m.shape != (grid.n_theta,) or a.shape != m.shape:
        raise ValueError(f"row_max and row_arg must be ({grid.n_theta},)")
    if beams < 1 or sep < 0:
        raise ValueError("beams >= 1 and min_separation >= 0")
    rows = []
    for _ in range(beams):
        i = int(m.argmax())                              # first occurrence: the lowest row on ties
        if m[i] <= 0:
            raise ValueError(f"only {len(rows)} rows hold votes {sep} rows apart, {beams} beams were asked for")
        rows.append((i, int(m[i])))
        m[max(0, i - sep):i + sep + 1] = 0
    rows.sort()
    idx = np.array([i for i, _ in rows], np.int64)
    return grid.theta()[idx], grid.h_centre(a[idx]), np.array([v for _, v in rows], np.int64)


def fit_lines(counts, sums, incl, height):
    """The least-squares line z = height - tan(incl) d of every beam from its moments, fp64:
    slope = (n Sdz - Sd Sz) / (n Sdd - Sd^2), height = (Sz - slope Sd) / n, incl = atan(-slope).  A beam with n < 2 or a
    zero denominator keeps (incl[k], height[k]).  -> (incl, height, kept: the ids of the beams that kept their value)."""
    incl, height = np.array(incl, np.float64), np.array(height, np.float64)
    kept = []
    for k in range(len(incl)):
        n = float(counts[k])
        sd, sz, sdd, sdz = (float(v) for v in sums[k])
        den = n * sdd - sd * sd
        if n < 2 or den == 0.0:
            kept.append(k)
            continue
        slope = (n * sdz - sd * sz) / den
        height[k] = (sz - slope * sd) / n
        incl[k] = math.atan(-slope)
    return incl, height, kept


@dataclasses.dataclass
class SensorTables:
    """height [m] and incl [rad, positive downwards] per beam, top beam first (float64 arrays); votes: each beam's Hough peak;
    support: the returns its line was fitted to (empty when the tables were not refined); grid: the HoughGrid they came from."""
    height: np.ndarray
    incl: np.ndarray
    votes: np.ndarray
    support: np.ndarray
    grid: HoughGrid

    def to_dict(self):
        return {"height": [float(v) for v in self.height], "incl": [float(v) for v in self.incl],
                "votes": [int(v) for v in self.votes], "support": [int(v) for v in self.support],
                "grid": dataclasses.asdict(self.grid)}

    @classmethod
    def from_dict(cls, d):
        return cls(np.array(d["height"], np.float64), np.array(d["incl"], np.float64), np.array(d["votes"], np.int64),
                   np.array(d["support"], np.int64), HoughGrid(**d["grid"]))

    def save(self, path):
        with open(path, "w") as f:
            f.write(json.dumps(self.to_dict(), sort_keys=True) + "\n")

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_dict(json.load(f))


# ---- device ---------------------------------------------------------------------------------------------------------
def _iter_clouds(clouds, lengths):
    if torch.is_tensor(clouds) and clouds.dim() == 3:
        if lengths is None:
            yield from clouds.unbind(0)
        else:
            ls = [int(v) for v in torch.as_tensor(lengths).tolist()]
            if len(ls) != clouds.shape[0] or any(v < 0 or v > clouds.shape[1] for v in ls):
                raise ValueError("lengths do not match the padded clouds")
            for i, n in enumerate(ls):
                yield clouds[i, :n]
        return
    if lengths is not None:
        raise ValueError("lengths is only meaningful for a padded tensor")
    for c in ([clouds] if (torch.is_tensor(clouds) or isinstance(clouds, np.ndarray)) else clouds):
        yield c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c))


def _device_chunks(clouds, lengths, device):
    """list (or any iterable, consumed one cloud at a time) of (n_i, >= 3) tensors / arrays, or a padded (N, P, >= 3) tensor with
    optional lengths (the packing of metrics.chamfer_pairs; empty clouds are fine here) -> fp32 device tensors (n, >= 3) of at most
    _CHUNK_POINTS points each (a cloud alone in its chunk keeps its columns: the kernel takes the stride)."""
    def joined(parts):
        return parts[0].contiguous() if len(parts) == 1 else torch.cat([q[:, :3] for q in parts], 0).contiguous()
    chunk, held = [], 0
    for c in _iter_clouds(clouds, lengths):
        if c.dim() != 2 or c.shape[1] < 3:
            raise ValueError("every cloud must be (n, >= 3)")
        if not c.shape[0]:
            continue
        for part in c.detach().to(device=device, dtype=torch.float32).split(_CHUNK_POINTS):
            if held + part.shape[0] > _CHUNK_POINTS and chunk:
                yield joined(chunk)
                chunk, held = [], 0
            chunk.append(part)
            held += part.shape[0]
    if chunk:
        yield joined(chunk)


def pack(points, d_min=2.0, d_max=90.0):
    """rldm_hough_pack: (n, >= 3) fp32 device points -> (n, 2) fp32 device pairs (d, z); d = -1 marks an invalid point."""
    if not points.is_cuda:
        raise RuntimeError("points must live on the GPU (rangeldm_amd has no CPU path)")
    pts = points.detach().float().contiguous()
    out = torch.empty((pts.shape[0], 2), dtype=torch.float32, device=pts.device)
    _lib.check(_lib.lib().rldm_hough_pack(pts.data_ptr(), pts.shape[0], pts.shape[1], float(d_min), float(d_max), out.data_ptr(),
                                          _lib.stream_ptr(pts.device)), "rldm_hough_pack")
    return out


def vote_shape(n, grid):
    """(rows of one workgroup, points of one slice) of a vote of n points into `grid`."""
    rows, slice_len = C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.lib().rldm_hough_vote_shape(int(n), int(grid.n_theta), int(grid.n_h), C.byref(rows), C.byref(slice_len)),
               "rldm_hough_vote_shape")
    return rows.value, slice_len.value


class HoughAccumulator:
    """The (n_theta, n_h) vote counters of `grid` on `device`.  add() packs clouds and votes them in; votes() / row_peaks()
    read the state.  `points` is the number of valid returns voted so far, kept on the host: add raises OverflowError before
    it reaches 2^32, so no uint32 counter can wrap (a return votes at most once per row)."""

    def __init__(self, grid, device="cuda"):
        _lib.require_gpu()
        self.grid = grid
        self.device = torch.device(device)
        self.points = 0
        self._acc = torch.zeros((grid.n_theta, grid.n_h), dtype=torch.int32, device=self.device)
        self._tan = torch.from_numpy(grid.tan_table()).to(self.device)

    def add_packed(self, packed):
        """Vote (n, 2) device pairs of pack(); returns the number of valid points among them."""
        valid = int((packed[:, 0] >= 0).sum().item())
        if self.points + valid >= POINT_LIMIT:
            raise OverflowError(f"{self.points} + {valid} valid points: a uint32 vote counter could wrap at 2^32")
        g = self.grid
        _lib.check(_lib.lib().rldm_hough_vote(packed.data_ptr(), packed.shape[0], self._tan.data_ptr(), int(g.n_theta),
                                              float(np.float32(g.h_min)), float(g.inv_dh()), int(g.n_h), self._acc.data_ptr(),
                                              _lib.stream_ptr(self.device)), "rldm_hough_vote")
        self.points += valid
        return valid

    def add(self, clouds, lengths=None):
        for pts in _device_chunks(clouds, lengths, self.device):
            self.add_packed(pack(pts, self.grid.d_min, self.grid.d_max))
        return self

    def votes(self):
        """The counters: a uint32 device tensor (n_theta, n_h) sharing the accumulator's memory."""
        return self._acc.view(torch.uint32)

    def row_peaks(self):
        """Per row (largest count, lowest bin attaining it): two int64 device tensors (n_theta,); a zero row gives (0, 0)."""
        g = self.grid
        mx = torch.empty((g.n_theta,), dtype=torch.int32, device=self.device)
        arg = torch.empty((g.n_theta,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().rldm_hough_row_max(self._acc.data_ptr(), int(g.n_theta), int(g.n_h), mx.data_ptr(), arg.data_ptr(),
                                                 _lib.stream_ptr(self.device)), "rldm_hough_row_max")
        return mx.long() & 0xFFFFFFFF, arg.long()


def assign(packed, cand, tol):
    """rldm_hough_assign: (n, 2) device pairs, (beams, 2) fp32 candidates (tan_k, h_k) -> int16 device ids (n,)."""
    cand = torch.as_tensor(np.ascontiguousarray(cand, np.float32)).to(packed.device)
    ids = torch.empty((packed.shape[0],), dtype=torch.int16, device=packed.device)
    _lib.check(_lib.lib().rldm_hough_assign(packed.data_ptr(), packed.shape[0], cand.data_ptr(), cand.shape[0], _tol(tol),
                                            ids.data_ptr(), _lib.stream_ptr(packed.device)), "rldm_hough_assign")
    return ids


def moments(packed, ids, beams):
    """rldm_hough_moments: -> (counts int64 (beams,), sums fp64 (beams, 4) = sum d, sum z, sum d^2, sum d z), device tensors;
    fixed summation order: two calls give the same bits."""
    if not 1 <= int(beams) <= _lib.RLDM_HOUGH_MAX_BEAMS:
        raise ValueError(f"beams must be in 1 .. {_lib.RLDM_HOUGH_MAX_BEAMS}")
    counts = torch.empty((beams,), dtype=torch.int64, device=packed.device)
    sums = torch.empty((beams, 4), dtype=torch.float64, device=packed.device)
    _lib.check(_lib.lib().rldm_hough_moments(packed.data_ptr(), ids.data_ptr(), packed.shape[0], int(beams), counts.data_ptr(),
                                             sums.data_ptr(), _lib.stream_ptr(packed.device)), "rldm_hough_moments")
    return counts, sums


def refine_beams(clouds, incl, height, tol, lengths=None, d_min=2.0, d_max=90.0, device="cuda"):
    """Assign every return to the nearest of the beams (incl, height) in tangent space (residual < tol) and fit each beam's
    line in closed form (fit_lines).  -> (incl, height, support, kept): fp64 tables, the returns behind each fit, and the ids
    of the beams that kept their input value (fewer than 2 returns, or all at one distance)."""
    _lib.require_gpu()
    cand = candidates(incl, height)
    beams = len(cand)
    counts, sums = np.zeros(beams, np.int64), np.zeros((beams, 4))
    for pts in _device_chunks(clouds, lengths, torch.device(device)):
        packed = pack(pts, d_min, d_max)
        c, s = moments(packed, assign(packed, cand, tol), beams)
        counts += c.cpu().numpy()
        sums += s.cpu().numpy()
    incl, height, kept = fit_lines(counts, sums, incl, height)
    return incl, height, counts, kept


def refine_beams_host(clouds, incl, height, tol, d_min=2.0, d_max=90.0):
    """refine_beams over the host statements."""
    cand = candidates(incl, height)
    packed = pack_host(clouds, d_min, d_max)
    counts, sums = moments_host(packed, assign_host(packed, cand, tol), len(cand))
    incl, height, kept = fit_lines(counts, sums, incl, height)
    return incl, height, counts, kept


def tables_from_peaks(peaks, refine_fn, clouds, beams, grid, min_separation, refine, tol):
    sep = 4 if min_separation is None else int(min_separation)
    incl, height, votes = pick_beams(peaks[0], peaks[1], beams, sep, grid)
    support = np.zeros(0, np.int64)
    if refine:
        tol = 2.0 * grid.theta_step if tol is None else tol
        incl, height, support, _ = refine_fn(clouds, incl, height, tol, d_min=grid.d_min, d_max=grid.d_max)
    return SensorTables(np.asarray(height, np.float64), np.asarray(incl, np.float64), votes, support, grid)


def estimate_sensor(clouds, beams, grid=None, min_separation=None, refine=True, tol=None, device="cuda"):
    """height / incl tables of a `beams`-beam sensor from a list of its sweeps ((n_i, >= 3) tensors or arrays; moved to
    `device`).  grid: HoughGrid.default() unless given; min_separation: rows suppressed either side of a picked row (4); tol:
    the tangent-space residual a return may have to count for a beam's fit (2 theta_step).  refine=False returns the Hough
    stage's bin centres.  -> SensorTables."""
    grid = HoughGrid.default() if grid is None else grid
    clouds = [clouds] if (torch.is_tensor(clouds) or isinstance(clouds, np.ndarray)) and clouds.ndim == 2 else list(clouds)
    acc = HoughAccumulator(grid, device).add(clouds)
    mx, arg = acc.row_peaks()

    def refine_fn(c, i, h, t, d_min, d_max):
        return refine_beams(c, i, h, t, d_min=d_min, d_max=d_max, device=device)
    return tables_from_peaks((mx.cpu().numpy(), arg.cpu().numpy()), refine_fn, clouds, beams, grid, min_separation, refine, tol)


def estimate_sensor_host(clouds, beams, grid=None, min_separation=None, refine=True, tol=None):
    """estimate_sensor over the host statements (numpy, one core): the tests' reference, and a GPU-free way to the tables."""
    grid = HoughGrid.default() if grid is None else grid
    clouds = _host_clouds(clouds)
    peaks = row_peaks_host(hough_votes_host(clouds, grid))
    return tables_from_peaks(peaks, refine_beams_host, clouds, beams, grid, min_separation, refine, tol)
