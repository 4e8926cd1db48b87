"""BEV-histogram evaluation on the GPU: the host-side mirror of
metrics/metrics/histogram/{histogram.py, dist_helper.py, mmd.py, jsd.py} -- same function names and argument meaning,
device tensors in, librangeldm_hip.so (rangeldm_amd/csrc/metrics.hip) underneath.  No CPU fallback.

    hists = point_cloud_to_histogram(160, 100, clouds)            # list of (n_i, >= 3) device tensors -> (S, 100, 100)
    jsd   = jsd_2d(model_hists, data_hists)
    mmd   = compute_mmd(data_hists, model_hists)                  # gaussian kernel, sigma = 0.5, is_hist=True

Reconstruction metrics (rangeldm_amd/csrc/chamfer.hip): chamfer_distance (pytorch3d call shape), nearest_sq_dists,
range_errors (MAE / PSNR / range MAE sums) and beam_upsample (the nearest / bicubic baselines).

Nearest neighbour with its index (rangeldm_amd/csrc/nn_index.hip): nearest_neighbours (d^2, the lowest index attaining it, and
per point the number of points that chose it), transfer (attributes carried across by those indices), and what is read off
them: match_counts / match_scores (precision, recall and F-score at distance thresholds), hausdorff, density_aware_chamfer
(Wu et al. 2021) and pair_scores (all of them and the CD from one search); nearest_neighbours_host, match_counts_host,
match_scores_host, hausdorff_host and density_aware_chamfer_host are the numpy statements.

K nearest neighbours (rangeldm_amd/csrc/knn.hip): knn_points / self_neighbours (pytorch3d's knn_points, exact, K <= 32),
estimate_normals (PCA over those neighbourhoods in fp64), chamfer_distance(x_normals=, y_normals=) (pytorch3d's loss_normals),
plane_scores (point-to-plane Chamfer distance and normal consistency per pair) and statistical_outliers (Open3D's rule);
knn_points_host, estimate_normals_host, normal_consistency_host, plane_scores_host and statistical_outliers_host are the numpy
statements.

Voxel occupancy (rangeldm_amd/csrc/voxel.hip): voxel_counts, per pair the distinct voxels of the result, of the target and of
both on a grid of `voxel` metres (a hash set per pair, filled with atomics alone), and voxel_scores, the IoU / precision /
recall / F1 of those integers; voxel_counts_host / voxel_scores_host are the numpy statements the device equals exactly.

Set-level generation metrics (chamfer.hip): chamfer_matrix (every cloud of one set against every cloud of another),
row_argmin (lowest index wins a tie) and generation_metrics (MMD-CD, COV-CD, 1-NNA-CD of Achlioptas et al. 2018 /
Yang et al. 2019); set_metrics_host is the numpy statement of the three reductions.

Earth Mover's Distance (rangeldm_amd/csrc/emd.hip): emd_matrix / emd_pairs, an epsilon-scaling auction between equal-size
clouds that returns the assignment and the dual prices with the value; generation_metrics(emd=True) adds MMD-EMD / COV-EMD /
1-NNA-EMD.

Frechet distance (rangeldm_amd/csrc/frechet.hip; metrics/metrics/fid/{lidargen_fid.py, fid_score.py}, the `--fid` command
over two folders of dumped activations): frechet_distance from an fp64 Gram product (gram_f64, on the fp64 MFMA) and its
singular values (singular_values, one-sided Jacobi); frechet_distance_host is the numpy statement, frd_indices and
load_activations the reference's index draw and file reading.

Kernel distance and precision / recall / density / coverage (rangeldm_amd/csrc/feature_metrics.hip): feature_scan, one row
scan of a set against another on the fp64 MFMA with per-row outputs only (no n x n matrix); knn_radii_sq, prdc and
kernel_distance on top of it; feature_scan_host, prdc_host and kernel_distance_host are the numpy statements.

Farthest point sampling (rangeldm_amd/csrc/fps.hip): farthest_point_sample, the sub-sampling of the protocol the set metrics
come from; subsample(method="fps") / subsample_batch put it behind the sub-sampling step of `evaluate generation`.
"""
import collections
import ctypes as C

import torch

from . import _lib

EMD_EPS = 2.0 ** -7         # metres: the auction's final epsilon (the value is within about this of the optimal matching)
EMD_MAX_POINTS = 2048       # RLDM_EMD_MAX_POINTS
FPS_BLOCK = 1024            # RLDM_FPS_BLOCK: lanes of the workgroup a cloud gets in farthest_point_sample
FPS_RESIDENT_POINTS = 65536     # RLDM_FPS_RESIDENT_POINTS: a cloud's first points, min-distance in registers
FPS_STAGED_POINTS = 12288   # RLDM_FPS_STAGED_POINTS: a cloud's first points, xyz staged in LDS (the others are re-read)
FPS_GROUP_POINTS = 4096     # RLDM_FPS_GROUP_POINTS: the re-read points go in groups of this many, four per lane
FPS_MAX_POINTS = 1048576    # RLDM_FPS_MAX_POINTS: the largest cloud farthest_point_sample takes


def _dev_u32(h):
    if not h.is_cuda:
        raise RuntimeError("histograms must live on the GPU (rangeldm_amd has no CPU path)")
    if h.dtype != torch.int32:
        h = h.to(torch.int32)
    return h.contiguous()


def point_cloud_to_histogram(field_size, bins, point_cloud, min_depth=None, max_depth=None):
    """histogram.py:4-18 for one cloud (n, >= 3) or a list of clouds; returns (S, bins, bins) int32 counts on the device.
    min_depth / max_depth: the `load_point_cloud_xyz` mask (mmd.py:39-44: 3 / 70 m for KITTI-360, 2 / 90 m for nuScenes),
    fused into the pass; None keeps every point."""
    clouds = [point_cloud] if torch.is_tensor(point_cloud) else list(point_cloud)
    if not clouds:
        raise ValueError("no point clouds")
    stride = clouds[0].shape[1]
    for c in clouds:
        if not c.is_cuda:
            raise RuntimeError("point clouds must live on the GPU (rangeldm_amd has no CPU path)")
        if c.dim() != 2 or c.shape[1] != stride or stride < 3:
            raise ValueError("every cloud must be (n, k) with the same k >= 3")
    _lib.require_gpu()
    dev = clouds[0].device
    pts = torch.cat([c.detach().float() for c in clouds], 0).contiguous()
    counts = torch.tensor([0] + [c.shape[0] for c in clouds], dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    hist = torch.empty((len(clouds), bins, bins), dtype=torch.int32, device=dev)
    lo = -1.0 if min_depth is None else float(min_depth)
    hi = float("inf") if max_depth is None else float(max_depth)
    _lib.check(_lib.lib().rldm_bev_histogram(pts.data_ptr(), counts.data_ptr(), len(clouds), stride, float(field_size),
                                             int(bins), lo, hi, hist.data_ptr(), _lib.stream_ptr(dev)),
               "rldm_bev_histogram")
    return hist


def jsd_2d(hists_p, hists_q):
    """jsd.py:90-101: Jensen-Shannon distance between the summed, normalised histogram sets (S, bins, bins)."""
    p, q = _dev_u32(hists_p), _dev_u32(hists_q)
    out = C.c_double(0.0)
    _lib.check(_lib.lib().rldm_hist_jsd(p.data_ptr(), p.shape[0], q.data_ptr(), q.shape[0], p.shape[1], C.byref(out),
                                        _lib.stream_ptr(p.device)), "rldm_hist_jsd")
    return out.value


def spectral_sq(hists_x, hists_y=None):
    """(nx, ny) fp32 table of `np.linalg.norm(pmf_i - pmf_j, 2) ** 2` (the distance inside dist_helper.gaussian)."""
    x = _dev_u32(hists_x)
    sym = hists_y is None
    y = x if sym else _dev_u32(hists_y)
    lam = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().rldm_hist_spectral_sq(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1],
                                                1 if sym else 0, lam.data_ptr(), _lib.stream_ptr(x.device)),
               "rldm_hist_spectral_sq")
    if sym:
        lam = lam + lam.t()
    return lam


def compute_mmd(samples1, samples2, kernel="gaussian", is_hist=True, sigma=0.5, return_terms=False):
    """dist_helper.py:156-172: s1 + s2 - 2 cross with the gaussian kernel on the spectral norm of pmf differences."""
    if kernel != "gaussian" or not is_hist:
        raise NotImplementedError("only compute_mmd(..., gaussian, is_hist=True), the call the reference's metric makes")
    x, y = _dev_u32(samples1), _dev_u32(samples2)
    out = (C.c_double * 4)()
    _lib.check(_lib.lib().rldm_hist_mmd(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1], float(sigma), out,
                                        _lib.stream_ptr(x.device)), "rldm_hist_mmd")
    return tuple(out) if return_terms else out[3]


def load_bin(path, columns=4, device="cuda"):
    """`np.fromfile(file, dtype=np.float32).reshape(-1, columns)` onto the device (mmd.py:40, :73)."""
    import numpy as np
    return torch.from_numpy(np.fromfile(path, dtype=np.float32).reshape(-1, columns)).to(device)


def evaluate_folders(sample_folder, data_files, nuscenes=False, limit=None):
    """calculate_jsd / calculate_mmd (jsd.py:64-101, mmd.py:96-125; *_nus variants :18-62 / :59-94): generated `.bin`
    files of `sample_folder` against the LiDAR sweeps `data_files` (the caller picks and shuffles them the way the
    reference does from its dataset directories).  Returns dict(jsd=..., mmd=...)."""
    import glob
    samples = sorted(glob.glob(f"{sample_folder}/*.bin"))[:limit]
    lo, hi = (2.0, 90.0) if nuscenes else (3.0, 70.0)
    model = point_cloud_to_histogram(160, 100, [load_bin(f, 4) for f in samples], lo, hi)
    data = point_cloud_to_histogram(160, 100, [load_bin(f, 5 if nuscenes else 4) for f in data_files[:len(samples)]], lo, hi)
    return {"jsd": jsd_2d(data, model), "mmd": compute_mmd(data, model)}


# ---- reconstruction metrics (rangeldm_amd/csrc/chamfer.hip) ---------------------------------------------------------
def _clouds(x, lengths, name):
    """Padded (N, P, >= 3) tensor (+ optional lengths) or a list of (n_i, >= 3) tensors -> list of (n_i, k) tensors.
    Shapes and emptiness are checked before anything touches the device."""
    if torch.is_tensor(x):
        if x.dim() != 3 or x.shape[2] < 3:
            raise ValueError(f"{name} must be (N, P, >= 3), got {tuple(x.shape)}")
        if lengths is None:
            clouds = list(x.unbind(0))
        else:
            ls = [int(v) for v in torch.as_tensor(lengths).tolist()]
            if len(ls) != x.shape[0] or any(v > x.shape[1] for v in ls):
                raise ValueError(f"{name}_lengths do not match {name}")
            clouds = [x[i, :n] for i, n in enumerate(ls)]
    else:
        if lengths is not None:
            raise ValueError(f"{name}_lengths is only meaningful for a padded tensor")
        clouds = list(x)
    if not clouds:
        raise ValueError(f"{name}: no point clouds")
    for c in clouds:
        if c.dim() != 2 or c.shape[1] < 3:
            raise ValueError(f"every cloud of {name} must be (n, >= 3)")
        if c.shape[0] == 0:
            raise ValueError(f"{name} holds an empty point cloud (the Chamfer distance is undefined)")
    return clouds


def _pack(clouds):
    """list of (n_i, k) device tensors -> (packed (sum n_i, k) fp32, offsets int32 [S + 1] on the device, k)."""
    for c in clouds:
        if not c.is_cuda:
            raise RuntimeError("point clouds must live on the GPU (rangeldm_amd has no CPU path)")
    k = min(c.shape[1] for c in clouds)
    pts = torch.cat([c.detach()[:, :k].float() for c in clouds], 0).contiguous()
    counts = torch.tensor([0] + [c.shape[0] for c in clouds], dtype=torch.int64).cumsum(0)
    if int(counts[-1]) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 points")
    return pts, counts.to(torch.int32).to(pts.device), k


def _nn(x, y, x_lengths, y_lengths):
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    xd = torch.empty(xp.shape[0], dtype=torch.float32, device=xp.device)
    yd = torch.empty(yp.shape[0], dtype=torch.float32, device=xp.device)
    _lib.check(_lib.lib().rldm_chamfer_nn(xp.data_ptr(), xo.data_ptr(), xk, yp.data_ptr(), yo.data_ptr(), yk, len(xs),
                                          xd.data_ptr(), yd.data_ptr(), _lib.stream_ptr(xp.device)), "rldm_chamfer_nn")
    return xd, xo, yd, yo, len(xs)


def nearest_sq_dists(x, y, x_lengths=None, y_lengths=None):
    """Per point of every cloud, the SQUARED distance to its nearest neighbour in the paired cloud of the other side (xyz
    only).  Returns (x_nn, y_nn): lists of 1-D fp32 device tensors, one per pair.  Each value is bit-equal to the fp32
    expression ((dx*dx + dy*dy) + dz*dz), dx = x_q - x_t, minimised over the other cloud."""
    xd, xo, yd, yo, _ = _nn(x, y, x_lengths, y_lengths)
    xs, ys = xo.cpu().tolist(), yo.cpu().tolist()
    return ([xd[a:b] for a, b in zip(xs[:-1], xs[1:])], [yd[a:b] for a, b in zip(ys[:-1], ys[1:])])


def chamfer_pairs(x, y, x_lengths=None, y_lengths=None):
    """(x_mean, y_mean): fp64 device tensors [N] -- per pair the mean over x of min_y d^2 and the mean over y of min_x d^2
    (fixed-order reductions: bit-identical run to run).  The Chamfer distance of pair p is x_mean[p] + y_mean[p]."""
    xd, xo, yd, yo, n = _nn(x, y, x_lengths, y_lengths)
    xm = torch.empty(n, dtype=torch.float64, device=xd.device)
    ym = torch.empty(n, dtype=torch.float64, device=xd.device)
    _lib.check(_lib.lib().rldm_chamfer_mean(xd.data_ptr(), xo.data_ptr(), yd.data_ptr(), yo.data_ptr(), n, xm.data_ptr(),
                                            ym.data_ptr(), _lib.stream_ptr(xd.device)), "rldm_chamfer_mean")
    return xm, ym


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, point_reduction="mean", batch_reduction="mean", norm=2,
                     x_normals=None, y_normals=None):
    """pytorch3d.loss.chamfer_distance with its defaults (ldm/convert_vae.py:262-271): padded (N, P, >= 3) tensors with
    optional lengths, or lists of (n_i, >= 3) device tensors; only xyz is used.  Returns (dist, loss_normals) like
    pytorch3d.  dist is an fp64 device scalar: batch_reduction "mean" averages the per-pair sums
    mean_x min_y d^2 + mean_y min_x d^2, "sum" adds them, None returns the (N,) vector.

    Without normals loss_normals is None.  With x_normals AND y_normals (each a padded (N, P, 3) tensor or a list of (n_i, 3)
    device tensors laid out like the clouds; estimate_normals gives such lists) it is pytorch3d's: per pair
    mean_i (1 - |cos(x_normals[i], y_normals[j(i)])|) + the mirror, j(i) the nearest point of the other cloud (the lowest
    index among ties: nearest_neighbours), cos = torch.nn.functional.cosine_similarity(eps=1e-6) in fp64; through the same
    batch_reduction.  dist then comes from that one search and has the bits it has without normals."""
    if point_reduction != "mean" or norm != 2:
        raise NotImplementedError("only point_reduction='mean', norm=2 (pytorch3d's defaults, the call the reference makes)")
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError(f"batch_reduction must be 'mean', 'sum' or None, got {batch_reduction!r}")
    if (x_normals is None) != (y_normals is None):
        raise ValueError("x_normals and y_normals must be given together")
    if x_normals is None:
        xm, ym = chamfer_pairs(x, y, x_lengths, y_lengths)
        parts = (xm + ym,)
    else:
        xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
        xn, yn = _normal_lists(x_normals, xs, "x_normals"), _normal_lists(y_normals, ys, "y_normals")
        r = _nn_index(xs, ys)
        parts = (_chamfer_means(r), _normal_consistency(r, xn, yn))
    if batch_reduction is None:
        return parts + (None,) * (2 - len(parts))
    parts = tuple(t.sum() if batch_reduction == "sum" else t.mean() for t in parts)
    return parts + (None,) * (2 - len(parts))


# ---- nearest neighbour with its index: F-score, Hausdorff, density-aware CD (rangeldm_amd/csrc/nn_index.hip) -------------
# the packed outputs of one rldm_nn_index call: per side d^2 (fp32), index into the pair's other cloud (int64), hits (int32),
# offsets (host list, pairs + 1 entries), and the device offsets rldm_chamfer_mean reads
_NNIndex = collections.namedtuple("_NNIndex", "xd xi xh xs yd yi yh ys xo yo")


def _nn_index(x, y, x_lengths=None, y_lengths=None):
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    dev = xp.device
    xd, yd = (torch.empty(t.shape[0], dtype=torch.float32, device=dev) for t in (xp, yp))
    xi, yi, xh, yh = (torch.empty(t.shape[0], dtype=torch.int32, device=dev) for t in (xp, yp, xp, yp))
    _lib.check(_lib.lib().rldm_nn_index(xp.data_ptr(), xo.data_ptr(), xk, yp.data_ptr(), yo.data_ptr(), yk, len(xs),
                                        xd.data_ptr(), xi.data_ptr(), yd.data_ptr(), yi.data_ptr(), xh.data_ptr(),
                                        yh.data_ptr(), _lib.stream_ptr(dev)), "rldm_nn_index")
    return _NNIndex(xd, xi.long(), xh, xo.cpu().tolist(), yd, yi.long(), yh, yo.cpu().tolist(), xo, yo)


def _chamfer_means(r):
    """x_mean + y_mean of chamfer_pairs (fp64 device (N,)) from the d^2 of one _nn_index search: the same bits."""
    n = len(r.xs) - 1
    xm = torch.empty(n, dtype=torch.float64, device=r.xd.device)
    ym = torch.empty(n, dtype=torch.float64, device=r.xd.device)
    _lib.check(_lib.lib().rldm_chamfer_mean(r.xd.data_ptr(), r.xo.data_ptr(), r.yd.data_ptr(), r.yo.data_ptr(), n, xm.data_ptr(),
                                            ym.data_ptr(), _lib.stream_ptr(xm.device)), "rldm_chamfer_mean")
    return xm + ym


def _per_pair(t, starts):
    return [t[a:b] for a, b in zip(starts[:-1], starts[1:])]


def _pair_ids(starts, device):
    counts = torch.tensor([b - a for a, b in zip(starts[:-1], starts[1:])], device=device)
    return torch.repeat_interleave(torch.arange(len(starts) - 1, device=device), counts)


def nearest_neighbours(x, y, x_lengths=None, y_lengths=None, return_hits=False):
    """nearest_sq_dists with the neighbour itself (pytorch3d's knn_points(K=1) in both directions).  Inputs as
    nearest_sq_dists takes them; returns (x_d2, x_idx, y_d2, y_idx), each a list of one 1-D device tensor per pair:

        x_d2[p][i]   fp32, the bits nearest_sq_dists gives: min over the points t of y_p of ((dx*dx + dy*dy) + dz*dz)
        x_idx[p][i]  int64, the LOWEST index j of y_p whose d^2 has exactly those bits (it indexes y_p, or any tensor laid
                     out like it, directly: see transfer)
        y_d2, y_idx  the mirror: the points of y_p against x_p

    return_hits=True appends (x_hits, y_hits), int32: y_hits[p][j] is the number of points of x_p whose x_idx is j, and
    x_hits the mirror (so y_hits[p].sum() == len(x_p)).  Everything is exact: it equals nearest_neighbours_host bit for bit
    and does not depend on the other pairs of the call or on how the kernel splits a cloud."""
    r = _nn_index(x, y, x_lengths, y_lengths)
    out = (_per_pair(r.xd, r.xs), _per_pair(r.xi, r.xs), _per_pair(r.yd, r.ys), _per_pair(r.yi, r.ys))
    return out + (_per_pair(r.xh, r.xs), _per_pair(r.yh, r.ys)) if return_hits else out


def transfer(values, idx):
    """Carry per-point attributes (remission, a SemanticKITTI label, ...) from the y clouds onto the x clouds: `values` is a
    list of (m_p, ...) tensors that live on the points of y_p, `idx` the x_idx of nearest_neighbours; the result is the list
    of (n_p, ...) gathers values[p][idx[p]]."""
    if len(values) != len(idx):
        raise ValueError(f"{len(values)} value tensors against {len(idx)} index tensors")
    return [v[i] for v, i in zip(values, idx)]


def _tau_values(taus):
    """`taus` (a number or a sequence of them) as a list of floats; ValueError unless every one is positive and finite as an
    fp32 number (the comparison is d^2 <= float32(tau) * float32(tau))."""
    import math
    import numpy as np
    try:
        vals = [float(t) for t in (taus if isinstance(taus, (list, tuple)) else np.atleast_1d(taus).tolist())]
    except (TypeError, ValueError):
        raise ValueError(f"tau must be positive, finite numbers, got {taus!r}") from None
    if not vals:
        raise ValueError("no distance threshold given")
    for v in vals:
        with np.errstate(over="ignore"):
            v32 = float(np.float32(v)) if math.isfinite(v) else v
        if not (v32 > 0.0 and math.isfinite(v32)):
            raise ValueError(f"tau must be positive and finite (as fp32), got {v!r}")
    return vals


def _tau_squares(taus):
    """float32(tau) * float32(tau), one fp32 multiply each, as an fp32 numpy array."""
    import numpy as np
    t = np.asarray(_tau_values(taus), np.float32)
    with np.errstate(over="ignore", under="ignore"):
        return t * t


def _alpha_value(alpha):
    import math
    if alpha is None:
        raise ValueError("alpha is required: the paper's 1000 is for unit-normalised shapes, there is no canonical value in metres")
    try:
        v = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"alpha must be a positive, finite number, got {alpha!r}") from None
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"alpha must be positive and finite, got {alpha!r}")
    return v


def _match_counts(r, taus):
    t2 = torch.from_numpy(_tau_squares(taus)).to(r.xd.device)
    n = len(r.xs) - 1
    out = torch.zeros((len(t2), 2, n), dtype=torch.int64, device=r.xd.device)
    for side, (d, starts) in enumerate(((r.xd, r.xs), (r.yd, r.ys))):
        # integer adds: exact, whatever order index_add_ takes them in
        out[:, side].index_add_(1, _pair_ids(starts, d.device), (d[None, :] <= t2[:, None]).long())
    return out.permute(2, 0, 1).contiguous()


def _hausdorff(r):
    n = len(r.xs) - 1
    # a maximum is order-free; the fp64 square root is taken on the host, where it is correctly rounded
    mx = torch.stack([torch.zeros(n, dtype=torch.float32, device=d.device).scatter_reduce_(0, _pair_ids(starts, d.device), d, "amax")
                      for d, starts in ((r.xd, r.xs), (r.yd, r.ys))], 1)
    import numpy as np
    h = torch.from_numpy(np.sqrt(mx.cpu().numpy().astype(np.float64)))      # (numpy's sqrt: IEEE, the host statement's)
    return torch.cat([h, h.max(1, keepdim=True).values], 1).to(r.xd.device)


def _dcd(r, alpha):
    a = _alpha_value(alpha)
    out = []
    for xd, xi, xh, yd, yi, yh in zip(*(_per_pair(t, s) for t, s in ((r.xd, r.xs), (r.xi, r.xs), (r.xh, r.xs),
                                                                    (r.yd, r.ys), (r.yi, r.ys), (r.yh, r.ys)))):
        tx = 1.0 - torch.exp(-(a * xd.double())) / yh[xi].double()
        ty = 1.0 - torch.exp(-(a * yd.double())) / xh[yi].double()
        out.append(0.5 * (tx.sum() / tx.shape[0] + ty.sum() / ty.shape[0]))
    return torch.stack(out)


def _match_ratios(counts, points, where):
    """precision, recall, fscore (fp64) from the matched counts (N, T, 2) and the cloud sizes (N, 2), torch or numpy alike."""
    f = counts.double() if torch.is_tensor(counts) else counts.astype("float64")
    s = points.double() if torch.is_tensor(points) else points.astype("float64")
    p, q = f[:, :, 0] / s[:, None, 0], f[:, :, 1] / s[:, None, 1]
    return {"precision": p, "recall": q, "fscore": where(p + q > 0, 2.0 * p * q / (p + q), 0.0 * p)}


def match_counts(x, y, taus, x_lengths=None, y_lengths=None):
    """Per pair and distance threshold tau the number of points within tau of the other cloud: an int64 device tensor
    (N, len(taus), 2), [p, k] = (points of x_p with d^2 <= t2, points of y_p with d^2 <= t2), t2 = float32(tau) * float32(tau)
    (one fp32 multiply) compared with the exact fp32 d^2 of nearest_neighbours: the integers equal match_counts_host.
    `taus` is a number or a sequence; every tau must be positive and finite (ValueError)."""
    _tau_values(taus)
    return _match_counts(_nn_index(x, y, x_lengths, y_lengths), taus)


def _match_scores(r, taus):
    counts = _match_counts(r, taus)
    points = torch.tensor([[b - a for a, b in zip(s[:-1], s[1:])] for s in (r.xs, r.ys)], device=counts.device).t()
    return {"tau": _tau_values(taus), **_match_ratios(counts, points, torch.where), "counts": counts, "points": points}


def match_scores(x, y, taus, x_lengths=None, y_lengths=None):
    """F-score at distance thresholds (Tatarchenko et al. 2019; Knapitsch et al. 2017) of result clouds x against their
    targets y.  A dict: "tau" the thresholds, "precision", "recall", "fscore" fp64 device tensors (N, len(taus)), "counts"
    the integers of match_counts and "points" the cloud sizes, int64 (N, 2):

        precision = matched_x / n_x      recall = matched_y / n_y      fscore = 2 p r / (p + r), 0 when p + r == 0

    Precision is about the result (the share of it within tau of the target), recall about the target.  Arguments and errors
    as match_counts."""
    _tau_values(taus)
    return _match_scores(_nn_index(x, y, x_lengths, y_lengths), taus)


def hausdorff(x, y, x_lengths=None, y_lengths=None):
    """Hausdorff distances per pair: an fp64 device tensor (N, 3), row p = (x_to_y, y_to_x, symmetric).  x_to_y is the
    fp64 square root of the largest fp32 d^2 of the points of x_p to their nearest neighbours in y_p (the worst point, which
    a mean hides), y_to_x the mirror, symmetric the larger of the two.  Exact given the d^2: it equals hausdorff_host."""
    return _hausdorff(_nn_index(x, y, x_lengths, y_lengths))


def density_aware_chamfer(x, y, alpha=None, x_lengths=None, y_lengths=None):
    """Density-aware Chamfer distance (Wu et al., NeurIPS 2021) per pair: an fp64 device tensor (N,).  With d^2_i the
    squared distance of point i of x_p to its nearest neighbour j(i) in y_p, e^2_j and i(j) the mirror, and y_hits[j] /
    x_hits[i] the number of points that chose j / i as their neighbour (nearest_neighbours(return_hits=True)):

        dcd = 1/2 [ mean_i (1 - exp(-alpha * d^2_i) / y_hits[j(i)]) + mean_j (1 - exp(-alpha * e^2_j) / x_hits[i(j)]) ]

    THIS variant puts the SQUARED distance in the exponent and has NO size-ratio factor (published code differs on both:
    some uses the unsquared distance, some scales a term by n_x / n_y when the clouds differ in size).  CD is blind to many
    result points collapsing onto one target point; here each of them earns only 1 / hits of the credit.  Every term lies
    in [0, 1] (a point's own hit count is at least 1).  fp64 throughout, alpha * d^2 included; the means are fixed-order sums.
    `alpha` has no default (ValueError when missing): the paper's 1000 is for unit-normalised shapes and there is no
    canonical value in metres; it must be positive and finite."""
    _alpha_value(alpha)
    return _dcd(_nn_index(x, y, x_lengths, y_lengths), alpha)


def pair_scores(x, y, taus=None, alpha=None, x_lengths=None, y_lengths=None):
    """Everything the nearest-neighbour search of result clouds x against targets y gives, from ONE search: a dict with "cd"
    (fp64 device (N,), the bits chamfer_pairs' x_mean + y_mean has: the same d^2 through the same fixed-order means) and,
    with `taus`, "match" (match_scores' dict) and "hausdorff" (hausdorff's tensor); with `alpha`, "dcd"."""
    if taus is not None:
        _tau_values(taus)
    if alpha is not None:
        _alpha_value(alpha)
    r = _nn_index(x, y, x_lengths, y_lengths)
    out = {"cd": _chamfer_means(r)}
    if taus is not None:
        out.update(match=_match_scores(r, taus), hausdorff=_hausdorff(r))
    if alpha is not None:
        out["dcd"] = _dcd(r, alpha)
    return out


def _nn_host_one(q, t):
    """(d2 fp32, idx int64) of the points of q against t: brute force, a block of rows at a time (about 2^20 distances, so a
    5 000 x 5 000 pair never holds more than 4 MB per temporary)."""
    import numpy as np
    q, t = (np.ascontiguousarray(np.asarray(c)[:, :3].astype(np.float32)) for c in (q, t))
    tx, ty, tz = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    d2, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int64)
    step = max(1, (1 << 20) // len(t))
    for lo in range(0, len(q), step):
        c = q[lo:lo + step]
        dx, dy, dz = c[:, 0:1] - tx, c[:, 1:2] - ty, c[:, 2:3] - tz
        d = (dx * dx + dy * dy) + dz * dz
        j = d.argmin(1)                                  # the first minimum: the lowest index
        idx[lo:lo + step] = j
        d2[lo:lo + step] = d[np.arange(len(c)), j]
    return d2, idx


def nearest_neighbours_host(x, y, return_hits=False):
    """The numpy statement of nearest_neighbours: lists of (n_i, >= 3) arrays (or one array per side: one pair) -> lists of
    arrays.  fp32 brute force with the kernel's expression ((dx*dx + dy*dy) + dz*dz), np.argmin (the first minimum), and
    np.bincount for the hits (int32)."""
    import numpy as np
    xs, ys = _voxel_host_clouds(x, "x"), _voxel_host_clouds(y, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    fwd = [_nn_host_one(a, b) for a, b in zip(xs, ys)]
    bwd = [_nn_host_one(b, a) for a, b in zip(xs, ys)]
    out = ([f[0] for f in fwd], [f[1] for f in fwd], [b[0] for b in bwd], [b[1] for b in bwd])
    if not return_hits:
        return out
    return out + ([np.bincount(b[1], minlength=len(a)).astype(np.int32) for a, b in zip(xs, bwd)],
                  [np.bincount(f[1], minlength=len(b)).astype(np.int32) for b, f in zip(ys, fwd)])


def match_counts_host(x, y, taus):
    """The numpy statement of match_counts: int64 (N, len(taus), 2)."""
    import numpy as np
    t2 = _tau_squares(taus)
    xd, _, yd, _ = nearest_neighbours_host(x, y)
    return np.array([[[int((a <= t).sum()), int((b <= t).sum())] for t in t2] for a, b in zip(xd, yd)], np.int64)


def match_scores_host(x, y, taus):
    """The numpy statement of match_scores: the same dict with numpy arrays."""
    import numpy as np
    counts = match_counts_host(x, y, taus)
    points = np.array([[len(a), len(b)] for a, b in zip(_voxel_host_clouds(x, "x"), _voxel_host_clouds(y, "y"))], np.int64)
    with np.errstate(invalid="ignore"):
        return {"tau": _tau_values(taus), **_match_ratios(counts, points, np.where), "counts": counts, "points": points}


def hausdorff_host(x, y):
    """The numpy statement of hausdorff: fp64 (N, 3)."""
    import numpy as np
    xd, _, yd, _ = nearest_neighbours_host(x, y)
    h = np.sqrt(np.array([[a.max(), b.max()] for a, b in zip(xd, yd)], np.float64))
    return np.concatenate([h, h.max(1, keepdims=True)], 1)


def density_aware_chamfer_host(x, y, alpha=None):
    """The numpy statement of density_aware_chamfer: fp64 (N,)."""
    import numpy as np
    a = _alpha_value(alpha)
    xd, xi, yd, yi, xh, yh = nearest_neighbours_host(x, y, return_hits=True)
    out = []
    for p in range(len(xd)):
        tx = 1.0 - np.exp(-(a * xd[p].astype(np.float64))) / yh[p][xi[p]].astype(np.float64)
        ty = 1.0 - np.exp(-(a * yd[p].astype(np.float64))) / xh[p][yi[p]].astype(np.float64)
        out.append(0.5 * (tx.sum() / len(tx) + ty.sum() / len(ty)))
    return np.array(out, np.float64)


# ---- K nearest neighbours, PCA normals, point-to-plane CD, normal consistency, outliers (rangeldm_amd/csrc/knn.hip) ------
KNN_MAX_K = 32              # RLDM_KNN_MAX_K


def _knn_k(K):
    """`K` as an int; ValueError unless it is an integer in 1..KNN_MAX_K."""
    import numbers
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or not 1 <= int(K) <= KNN_MAX_K:
        raise ValueError(f"K must be an integer in 1..{KNN_MAX_K}, got {K!r}")
    return int(K)


def _knn(xs, ys, K, exclude_self):
    """One rldm_knn call, the clouds xs against ys (ys None: xs against themselves).  Returns the packed d2 (n, K) fp32 and
    idx (n, K) int32, the packed queries with their device offsets and stride, and the offsets as a host list."""
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = (xp, xo, xk) if ys is None else _pack(ys)
    d2 = torch.empty((xp.shape[0], K), dtype=torch.float32, device=xp.device)
    idx = torch.empty((xp.shape[0], K), dtype=torch.int32, device=xp.device)
    _lib.check(_lib.lib().rldm_knn(xp.data_ptr(), xo.data_ptr(), xk, yp.data_ptr(), yo.data_ptr(), yk, len(xs), K,
                                   1 if exclude_self else 0, d2.data_ptr(), idx.data_ptr(), _lib.stream_ptr(xp.device)),
               "rldm_knn")
    return d2, idx, xp, xo, xk, xo.cpu().tolist()


def knn_points(x, y, K, x_lengths=None, y_lengths=None):
    """pytorch3d's knn_points, exact: for every point of x_p its K nearest points of y_p.  Inputs as nearest_neighbours takes
    them, 1 <= K <= 32.  Returns (d2, idx), each a list with one entry per pair: d2[p] (n_p, K) fp32, idx[p] (n_p, K) int64.
    Row i holds the K points of y_p that are smallest in the order (d^2 bits, index), ascending in that order, with the fp32
    d^2 = ((dx*dx + dy*dy) + dz*dz) of nearest_sq_dists: equal distances go to the lower index, and K = 1 is
    nearest_neighbours' x_d2 / x_idx bit for bit.  Where y_p has fewer than K points the row ends in (+inf, -1).  Everything
    equals knn_points_host exactly and depends on the two clouds of the pair alone."""
    K = _knn_k(K)
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    d2, idx, _, _, _, starts = _knn(xs, ys, K, False)
    return _per_pair(d2, starts), _per_pair(idx.long(), starts)


def self_neighbours(x, K, x_lengths=None):
    """knn_points of every cloud against itself with the point itself left out (only itself: another point at the same
    coordinates is a neighbour at d^2 = 0).  A cloud of fewer than K + 1 points has rows that end in (+inf, -1)."""
    K = _knn_k(K)
    d2, idx, _, _, _, starts = _knn(_clouds(x, x_lengths, "x"), None, K, True)
    return _per_pair(d2, starts), _per_pair(idx.long(), starts)


def _knn_host_one(q, t, K, exclude_self):
    import numpy as np
    q, t = (np.ascontiguousarray(np.asarray(c)[:, :3].astype(np.float32)) for c in (q, t))
    if exclude_self and len(q) != len(t):
        raise ValueError("exclude_self needs clouds of equal sizes")
    tx, ty, tz = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    d2 = np.full((len(q), K), np.inf, np.float32)
    idx = np.full((len(q), K), -1, np.int64)
    step = max(1, (1 << 20) // len(t))
    for lo in range(0, len(q), step):
        c = q[lo:lo + step]
        dx, dy, dz = c[:, 0:1] - tx, c[:, 1:2] - ty, c[:, 2:3] - tz
        d = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((np.broadcast_to(np.arange(len(t)), d.shape), d), axis=-1)      # by d2, then by index
        if exclude_self:
            order = order[order != np.arange(lo, lo + len(c))[:, None]].reshape(len(c), len(t) - 1)
        order = order[:, :K]
        idx[lo:lo + len(c), :order.shape[1]] = order
        d2[lo:lo + len(c), :order.shape[1]] = np.take_along_axis(d, order, 1)
    return d2, idx


def knn_points_host(x, y, K, exclude_self=False):
    """The numpy statement of knn_points (exclude_self=True with y = x: of self_neighbours): lists of (n_i, >= 3) arrays (or
    one array per side: one pair) -> (d2, idx) lists of (n_i, K) fp32 / int64 arrays.  fp32 brute force with the kernel's
    expression ((dx*dx + dy*dy) + dz*dz), then np.lexsort((index, d2))[:K] per row; missing slots are (+inf, -1)."""
    K = _knn_k(K)
    xs, ys = _voxel_host_clouds(x, "x"), _voxel_host_clouds(y, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    out = [_knn_host_one(a, b, K, exclude_self) for a, b in zip(xs, ys)]
    return [o[0] for o in out], [o[1] for o in out]


def estimate_normals(x, K=16, x_lengths=None, return_eigenvalues=False):
    """Surface normals by PCA over the K nearest neighbours (self_neighbours): a list of (n_p, 3) fp64 device tensors.  Per
    point, in fp64: the covariance of the point and its neighbours about their centroid, divided by their number; the normal
    is the unit eigenvector of its smallest eigenvalue, oriented towards the sensor at the origin (n . p <= 0; when that is 0
    the first non-zero component is positive).  A point with fewer than two neighbours (a cloud of one or two points) gets
    zeros.  return_eigenvalues=True appends the list of (n_p, 3) ascending eigenvalues (lambda_0 / trace is the surface
    variation).  estimate_normals_host on the same indices is the numpy statement."""
    K = _knn_k(K)
    xs = _clouds(x, x_lengths, "x")
    _, idx, xp, xo, xk, starts = _knn(xs, None, K, True)
    normals = torch.empty((xp.shape[0], 3), dtype=torch.float64, device=xp.device)
    eig = torch.empty((xp.shape[0], 3), dtype=torch.float64, device=xp.device)
    _lib.check(_lib.lib().rldm_knn_normals(xp.data_ptr(), xo.data_ptr(), xk, len(xs), idx.data_ptr(), K, normals.data_ptr(),
                                           eig.data_ptr(), _lib.stream_ptr(xp.device)), "rldm_knn_normals")
    out = _per_pair(normals, starts)
    return (out, _per_pair(eig, starts)) if return_eigenvalues else out


def _normals_host_one(pts, idx):
    import numpy as np
    pts = np.asarray(pts)[:, :3].astype(np.float32).astype(np.float64)
    idx = np.asarray(idx).reshape(len(pts), -1)
    valid = (idx >= 0) & (idx < len(pts))
    w = np.concatenate([np.ones((len(pts), 1)), valid.astype(np.float64)], 1)             # the point itself, then its neighbours
    nb = np.concatenate([pts[:, None, :], pts[np.where(valid, idx, 0)]], 1)
    m = w.sum(1)
    cen = (nb * w[..., None]).sum(1) / m[:, None]
    d = (nb - cen[:, None, :]) * w[..., None]
    cov = np.einsum("nki,nkj->nij", d, d) / m[:, None, None]
    lam, vec = np.linalg.eigh(cov)                       # ascending
    n = vec[:, :, 0]
    dot = (n * pts).sum(1)
    nz = n != 0.0
    lead = np.take_along_axis(n, nz.argmax(1)[:, None], 1)[:, 0]
    flip = (dot > 0.0) | ((dot == 0.0) & (lead < 0.0))
    n = np.where(flip[:, None], -n, n) + 0.0
    few = m < 3
    n[few], lam[few] = 0.0, 0.0
    return n, lam


def estimate_normals_host(x, idx, return_eigenvalues=False):
    """The numpy statement of estimate_normals given the neighbour indices (self_neighbours' idx, or knn_points_host's with
    exclude_self): lists of (n_i, >= 3) arrays and of (n_i, K) index arrays (or one of each) -> a list of (n_i, 3) fp64
    normals.  Covariance in fp64, np.linalg.eigh, the same orientation rule."""
    import numpy as np
    xs = _voxel_host_clouds(x, "x")
    ids = [np.asarray(idx)] if len(xs) == 1 and np.asarray(idx[0]).ndim == 1 else [np.asarray(i) for i in idx]
    if len(ids) != len(xs) or any(len(i) != len(c) for i, c in zip(ids, xs)):
        raise ValueError("idx does not match x")
    out = [_normals_host_one(c, i) for c, i in zip(xs, ids)]
    return ([o[0] for o in out], [o[1] for o in out]) if return_eigenvalues else [o[0] for o in out]


def _normal_lists(normals, clouds, name):
    """A padded (N, P, 3) tensor or a list of (n_i, 3) tensors -> the list of (n_i, 3) fp64 device tensors that belongs to
    `clouds`; ValueError when the shapes do not match them."""
    if torch.is_tensor(normals):
        if normals.dim() != 3 or normals.shape[0] != len(clouds) or normals.shape[2] != 3 or \
                any(c.shape[0] > normals.shape[1] for c in clouds):
            raise ValueError(f"{name} must be (N, P, 3) like its clouds, got {tuple(normals.shape)}")
        out = [normals[i, :c.shape[0]] for i, c in enumerate(clouds)]
    else:
        out = list(normals)
        if len(out) != len(clouds) or any((not torch.is_tensor(n)) or tuple(n.shape) != (c.shape[0], 3) for n, c in zip(out, clouds)):
            raise ValueError(f"{name} must hold one (n_i, 3) tensor per cloud")
    for n in out:
        if not n.is_cuda:
            raise RuntimeError("normals must live on the GPU (rangeldm_amd has no CPU path)")
    return [n.detach().double() for n in out]


def _normal_consistency(r, xn, yn):
    """pytorch3d's loss_normals per pair (fp64 device (N,)) from one _nn_index search and the two sides' normals: each pair is
    reduced on its own, in a fixed order."""
    import torch.nn.functional as F
    out = []
    for nx, ny, xi, yi in zip(xn, yn, _per_pair(r.xi, r.xs), _per_pair(r.yi, r.ys)):
        tx = 1.0 - F.cosine_similarity(nx, ny[xi], dim=1, eps=1e-6).abs()
        ty = 1.0 - F.cosine_similarity(ny, nx[yi], dim=1, eps=1e-6).abs()
        out.append(tx.sum() / tx.shape[0] + ty.sum() / ty.shape[0])
    return torch.stack(out)


def _plane_term(a, b, bn, j):
    """mean over the points of a of ((a_i - b_j(i)) . bn_j(i))^2 in fp64, torch or numpy alike."""
    d, n = a - b[j], bn[j]
    s = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    return (s * s).sum() / a.shape[0]


def plane_scores(x, y, K=16, x_lengths=None, y_lengths=None):
    """What the distance to the nearest SAMPLE cannot tell apart, per pair: a dict of fp64 device (N,) tensors

        "cd"                  pair_scores' "cd" (the same bits)
        "cd_plane"            mean_i ((x_i - y_j(i)) . n_y[j(i)])^2 + mean_j ((y_j - x_i(j)) . n_x[i(j)])^2: the squared distance
                              to the tangent plane at the nearest point, which does not charge a point for lying on the right
                              surface between the other cloud's beams
        "normal_consistency"  chamfer_distance's loss_normals: mean_i (1 - |cos(n_x[i], n_y[j(i)])|) + the mirror

    j(i) / i(j) are nearest_neighbours' indices, n_x / n_y estimate_normals(K) of each side, all arithmetic fp64.  A pair's
    values do not depend on the other pairs of the call.  plane_scores_host is the numpy statement."""
    K = _knn_k(K)
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    xn, yn = estimate_normals(xs, K), estimate_normals(ys, K)
    r = _nn_index(xs, ys)
    plane = []
    for a, b, an, bn, xi, yi in zip(xs, ys, xn, yn, _per_pair(r.xi, r.xs), _per_pair(r.yi, r.ys)):
        a, b = a.detach()[:, :3].float().double(), b.detach()[:, :3].float().double()
        plane.append(_plane_term(a, b, bn, xi) + _plane_term(b, a, an, yi))
    return {"cd": _chamfer_means(r), "cd_plane": torch.stack(plane), "normal_consistency": _normal_consistency(r, xn, yn)}


def _cosine_host(a, b, eps=1e-6):
    import numpy as np
    na, nb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    return (a * b).sum(1) / (np.maximum(na, eps) * np.maximum(nb, eps))


def normal_consistency_host(x, y, x_normals, y_normals):
    """The numpy statement of chamfer_distance's loss_normals per pair: fp64 (N,)."""
    import numpy as np
    _, xi, _, yi = nearest_neighbours_host(x, y)
    out = []
    for nx, ny, i, j in zip(x_normals, y_normals, xi, yi):
        nx, ny = np.asarray(nx, np.float64), np.asarray(ny, np.float64)
        tx, ty = 1.0 - np.abs(_cosine_host(nx, ny[i])), 1.0 - np.abs(_cosine_host(ny, nx[j]))
        out.append(tx.sum() / len(tx) + ty.sum() / len(ty))
    return np.array(out, np.float64)


def plane_scores_host(x, y, K=16):
    """The numpy statement of plane_scores: the same dict with fp64 numpy arrays (normals from estimate_normals_host on
    knn_points_host's self-excluding indices)."""
    import numpy as np
    K = _knn_k(K)
    xs, ys = _voxel_host_clouds(x, "x"), _voxel_host_clouds(y, "y")
    xn = estimate_normals_host(xs, knn_points_host(xs, xs, K, exclude_self=True)[1])
    yn = estimate_normals_host(ys, knn_points_host(ys, ys, K, exclude_self=True)[1])
    xd, xi, yd, yi = nearest_neighbours_host(xs, ys)
    cd = [a.astype(np.float64).sum() / len(a) + b.astype(np.float64).sum() / len(b) for a, b in zip(xd, yd)]
    plane = []
    for a, b, an, bn, i, j in zip(xs, ys, xn, yn, xi, yi):
        a, b = (c[:, :3].astype(np.float32).astype(np.float64) for c in (a, b))
        plane.append(_plane_term(a, b, bn, i) + _plane_term(b, a, an, j))
    return {"cd": np.array(cd, np.float64), "cd_plane": np.array(plane, np.float64),
            "normal_consistency": normal_consistency_host(xs, ys, xn, yn)}


def _std_ratio(std_ratio):
    import math
    try:
        v = float(std_ratio)
    except (TypeError, ValueError):
        raise ValueError(f"std_ratio must be a finite number, got {std_ratio!r}") from None
    if not math.isfinite(v):
        raise ValueError(f"std_ratio must be finite, got {std_ratio!r}")
    return v


def _outlier_rule(d2, idx, ratio, sqrt, where, zero):
    """(mask, mean neighbour distance per point, threshold) of one cloud from its self_neighbours rows and a zero array of
    their shape, torch or numpy alike."""
    valid = idx >= 0
    count = valid.sum(1)
    dist = sqrt(where(valid, d2, zero))                  # an empty slot (+inf, -1) adds nothing
    mean = dist.sum(1) / where(count > 0, count, count + 1)
    mu = mean.sum() / mean.shape[0]
    sd = sqrt(((mean - mu) * (mean - mu)).sum() / mean.shape[0])
    thr = mu + ratio * sd
    return mean > thr, mean, thr


def statistical_outliers(x, K=20, std_ratio=2.0, x_lengths=None, return_terms=False):
    """Open3D's remove_statistical_outlier rule (the isolated floating points a sampler leaves between objects): a list of
    bool device masks, True where a point's mean distance to its K nearest neighbours (self_neighbours; the fp64 mean over the
    valid slots of sqrt(d^2)) exceeds the cloud's mean of those means plus std_ratio times their population standard
    deviation.  return_terms=True appends the lists of per-point means and of the clouds' thresholds (fp64).
    statistical_outliers_host is the numpy statement."""
    K, ratio = _knn_k(K), _std_ratio(std_ratio)
    d2, idx, _, _, _, starts = _knn(_clouds(x, x_lengths, "x"), None, K, True)
    out = [_outlier_rule(d.double(), i, ratio, torch.sqrt, torch.where, torch.zeros_like(d, dtype=torch.float64)) for d, i in zip(_per_pair(d2, starts), _per_pair(idx, starts))]
    masks = [o[0] for o in out]
    return (masks, [o[1] for o in out], [o[2] for o in out]) if return_terms else masks


def statistical_outliers_host(x, K=20, std_ratio=2.0, return_terms=False):
    """The numpy statement of statistical_outliers: lists of (n_i, >= 3) arrays (or one array) -> a list of bool arrays."""
    import numpy as np
    K, ratio = _knn_k(K), _std_ratio(std_ratio)
    xs = _voxel_host_clouds(x, "x")
    d2, idx = knn_points_host(xs, xs, K, exclude_self=True)
    out = [_outlier_rule(d.astype(np.float64), i, ratio, np.sqrt, np.where, np.zeros(d.shape)) for d, i in zip(d2, idx)]
    masks = [o[0] for o in out]
    return (masks, [o[1] for o in out], [float(o[2]) for o in out]) if return_terms else masks


# ---- voxel occupancy: IoU / precision / recall / F1 of the occupied voxels (rangeldm_amd/csrc/voxel.hip) ------------------
VOXEL_HALF_RANGE = 1 << 20      # a voxel index q must satisfy -2^20 <= q < 2^20 on every axis
VOXEL_SCORES = ("iou", "precision", "recall", "f1")


def _voxel_size(voxel):
    """`voxel` as a float; ValueError unless it is positive and finite as an fp32 number (the kernel divides by float32(voxel))."""
    import math
    import numpy as np
    try:
        v = float(voxel)
    except (TypeError, ValueError):
        raise ValueError(f"voxel must be a positive, finite number, got {voxel!r}") from None
    with np.errstate(over="ignore"):
        v32 = float(np.float32(v)) if math.isfinite(v) else v
    if not (v32 > 0.0 and math.isfinite(v32)):
        raise ValueError(f"voxel must be positive and finite (as fp32), got {voxel!r}")
    return v


def _voxel_ratios(a, b, c):
    """The four scores from fp64 arrays / tensors of the counts (integers below 2^53: exact), one IEEE division each."""
    return {"iou": c / (a + b - c), "precision": c / a, "recall": c / b, "f1": 2.0 * c / (a + b)}


def voxel_counts(x, y, voxel=0.1, x_lengths=None, y_lengths=None):
    """Voxel-occupancy counts of result clouds x against their targets y: an int64 device tensor (N, 3), row p =
    (a, b, c) = (distinct voxels of x_p, distinct voxels of y_p, voxels in both).  Inputs as chamfer_pairs takes them (padded
    (N, P, >= 3) tensors with optional lengths, or lists of (n_i, >= 3) device tensors; only xyz is read).

        v = float32(voxel);  q(c) = floor(c / v), one correctly rounded fp32 division, then floor (fp32 denormals kept:
        floor(-1e-40 / 0.1) is -1);  a point's voxel is (q(x), q(y), q(z))

    A point is in range when its coordinates are finite and -2^20 <= q < 2^20 on every axis; a call holding ANY point out of
    range raises ValueError and reports nothing (the next call works normally).  The counts are integers: they do not depend
    on the order of the points or of the pairs, on the other pairs of the call, or on the kernel's chunking, and they equal
    voxel_counts_host exactly.  Argument errors (an empty cloud, mismatched pair counts, voxel <= 0 or non-finite) are
    ValueErrors raised before the device is touched."""
    v = _voxel_size(voxel)
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    counts = torch.empty((len(xs), 3), dtype=torch.int32, device=xp.device)
    L = _lib.lib()
    rc = L.rldm_voxel_counts(xp.data_ptr(), xo.data_ptr(), xk, yp.data_ptr(), yo.data_ptr(), yk, len(xs), v,
                             counts.data_ptr(), _lib.stream_ptr(xp.device))
    if rc == _lib.RLDM_VOXEL_RANGE:
        msg = L.rldm_last_error()
        raise ValueError(f"rldm_voxel_counts: {msg.decode() if msg else 'a point is out of range'}")
    _lib.check(rc, "rldm_voxel_counts")
    return counts.long()


def voxel_scores(x, y, voxel=0.1, x_lengths=None, y_lengths=None):
    """Occupancy scores of result clouds x against their targets y on a grid of `voxel` metres (0.1: Implicit LiDAR Network,
    TULIP and the tables after them).  A dict of fp64 device tensors (N,) and the counts of voxel_counts (int64 (N, 3)):

        iou = c / (a + b - c)      precision = c / a      recall = c / b      f1 = 2c / (a + b)

    each one fp64 division of the integers.  Precision is about the result x (how much of it is geometry the target has),
    recall about the target y (how much of it was hit at all).  Arguments and errors as voxel_counts."""
    counts = voxel_counts(x, y, voxel, x_lengths, y_lengths)
    f = counts.double()
    return {**_voxel_ratios(f[:, 0], f[:, 1], f[:, 2]), "counts": counts}


def _voxel_host_clouds(x, name):
    import numpy as np
    if (torch.is_tensor(x) or isinstance(x, np.ndarray)) and x.ndim == 2:
        x = [x]                                          # one cloud: one pair
    clouds = [np.asarray(c) for c in x]
    if not clouds:
        raise ValueError(f"{name}: no point clouds")
    for c in clouds:
        if c.ndim != 2 or c.shape[1] < 3:
            raise ValueError(f"every cloud of {name} must be (n, >= 3)")
        if c.shape[0] == 0:
            raise ValueError(f"{name} holds an empty point cloud")
    return clouds


def _voxel_keys_host(cloud, v32):
    """The distinct voxels of one cloud, each packed into one int64 (sorted): np.unique(axis=0) of floor(c / v)."""
    import numpy as np
    with np.errstate(all="ignore"):
        q = np.floor(cloud[:, :3].astype(np.float32) / v32)
    if not ((q >= -VOXEL_HALF_RANGE) & (q < VOXEL_HALF_RANGE)).all():        # (NaN fails both comparisons)
        raise ValueError(f"a point is out of range: a coordinate is NaN or inf, or floor(c / voxel) lies outside "
                         f"[-2^20, 2^20)")
    rows = np.unique(q.astype(np.int64), axis=0) + VOXEL_HALF_RANGE
    return rows[:, 0] | rows[:, 1] << 21 | rows[:, 2] << 42


def voxel_counts_host(x, y, voxel=0.1):
    """The numpy statement of voxel_counts: lists of (n_i, >= 3) arrays (or one array per side: one pair) -> int64 (N, 3).
    Per cloud `np.floor(c.astype(np.float32) / np.float32(voxel))`, np.unique(axis=0), and per pair the intersection of the
    two sets.  Raises the ValueErrors of voxel_counts, the one for a point out of range included."""
    import numpy as np
    v32 = np.float32(_voxel_size(voxel))
    xs, ys = _voxel_host_clouds(x, "x"), _voxel_host_clouds(y, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    out = np.empty((len(xs), 3), np.int64)
    for p, (cx, cy) in enumerate(zip(xs, ys)):
        kx, ky = _voxel_keys_host(cx, v32), _voxel_keys_host(cy, v32)
        out[p] = (len(kx), len(ky), len(np.intersect1d(kx, ky, assume_unique=True)))
    return out


def voxel_scores_host(x, y, voxel=0.1):
    """The numpy statement of voxel_scores: fp64 arrays iou, precision, recall, f1 (N,) and the int64 counts (N, 3)."""
    import numpy as np
    counts = voxel_counts_host(x, y, voxel)
    f = counts.astype(np.float64)
    return {**_voxel_ratios(f[:, 0], f[:, 1], f[:, 2]), "counts": counts}


# ---- set-level generation metrics: all-pairs Chamfer matrix, MMD-CD / COV-CD / 1-NNA-CD -------------------------------
def chamfer_matrix(x, y=None, x_lengths=None, y_lengths=None, return_directions=False):
    """CD[i][j] = mean_{q in x_i} min_{t in y_j} d^2 + mean_{t in y_j} min_{q in x_i} d^2 for EVERY cloud of x against every
    cloud of y: an fp64 device (nx, ny) tensor.  y=None is the symmetric case (x against itself: zero diagonal, CD equal to
    its transpose bit for bit).  Inputs as chamfer_distance takes them.  return_directions=True returns (xy, yx), the two
    terms.  Every entry is a fixed-order fp64 mean of fp32 minima that are bit-equal to the CPU expression, and depends on its
    two clouds alone: a block of rows computed on its own (x[a:b] against y) equals those rows of the whole matrix."""
    xs = _clouds(x, x_lengths, "x")
    ys = None if y is None else _clouds(y, y_lengths, "y")
    if y is None and y_lengths is not None:
        raise ValueError("y_lengths without y")
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = (xp, xo, xk) if ys is None else _pack(ys)
    nx, ny = len(xs), len(xs if ys is None else ys)
    xy = torch.empty((nx, ny), dtype=torch.float64, device=xp.device)
    yx = torch.empty_like(xy)
    _lib.check(_lib.lib().rldm_chamfer_matrix(xp.data_ptr(), xo.data_ptr(), xk, nx, yp.data_ptr(), yo.data_ptr(), yk, ny,
                                              1 if ys is None else 0, xy.data_ptr(), yx.data_ptr(), _lib.stream_ptr(xp.device)),
               "rldm_chamfer_matrix")
    return (xy, yx) if return_directions else xy + yx


def row_argmin(m, exclude_diag=False):
    """Per row of a device fp64 (n, m) matrix: (minimum, LOWEST column index attaining it) as fp64 / int32 device tensors.
    exclude_diag skips column r of row r (a cloud is not its own neighbour).  torch.argmin does not promise which index wins
    a tie; the set metrics are counts of argmins, so the rule is stated and kept here."""
    if m.dim() != 2 or m.shape[0] == 0 or m.shape[1] == 0:
        raise ValueError(f"m must be a non-empty (n, m) matrix, got {tuple(m.shape)}")
    if not m.is_cuda:
        raise RuntimeError("the matrix must live on the GPU (rangeldm_amd has no CPU path)")
    m = m.detach().to(torch.float64).contiguous()
    mn = torch.empty(m.shape[0], dtype=torch.float64, device=m.device)
    arg = torch.empty(m.shape[0], dtype=torch.int32, device=m.device)
    _lib.check(_lib.lib().rldm_matrix_row_argmin(m.data_ptr(), m.shape[0], m.shape[1], 1 if exclude_diag else 0,
                                                 mn.data_ptr(), arg.data_ptr(), _lib.stream_ptr(m.device)),
               "rldm_matrix_row_argmin")
    return mn, arg


def _mean_exact(values):
    """Correctly rounded mean of a 1-D device tensor (math.fsum on the host: no dependence on a reduction order)."""
    import math
    v = values.cpu().tolist()
    return math.fsum(v) / len(v)


def set_metrics(cd_gg, cd_gr, cd_rr, name="cd"):
    """MMD-CD, COV-CD and 1-NNA-CD from the three device fp64 Chamfer matrices: generated x generated (ng, ng), generated x
    reference (ng, nr), reference x reference (nr, nr).  Ties go to the lowest index (row_argmin).  `name` names the
    distance in the keys ("emd": mmd_emd, cov_emd, nna_emd, ...; the matrices are then emd_matrix's).
      mmd_cd   mean over reference clouds r of min_g CD[g][r]
      cov_cd   distinct reference clouds that are argmin_r CD[g][r] for some generated g, over nr
      nna_cd   leave-one-out 1-nearest-neighbour accuracy over the union ordered [G_0 .. G_{ng-1}, R_0 .. R_{nr-1}]: the
               fraction of clouds whose nearest OTHER cloud carries their own label (0.5 is ideal; nna_cd_gen / nna_cd_ref: the
               same over the generated / the reference clouds alone)."""
    ng, nr = cd_gr.shape
    if tuple(cd_gg.shape) != (ng, ng) or tuple(cd_rr.shape) != (nr, nr):
        raise ValueError(f"matrices of shapes {tuple(cd_gg.shape)}, {tuple(cd_gr.shape)}, {tuple(cd_rr.shape)} do not fit")
    mins, _ = row_argmin(cd_gr.t())
    _, covered = row_argmin(cd_gr)
    union = torch.cat([torch.cat([cd_gg, cd_gr], 1), torch.cat([cd_gr.t(), cd_rr], 1)], 0)
    _, nn = row_argmin(union, exclude_diag=True)
    same = (nn >= ng) == (torch.arange(ng + nr, device=nn.device) >= ng)
    right_gen, right_ref = int(same[:ng].sum()), int(same[ng:].sum())
    return {f"mmd_{name}": _mean_exact(mins), f"cov_{name}": int(torch.unique(covered).numel()) / nr,
            f"nna_{name}": (right_gen + right_ref) / (ng + nr), f"nna_{name}_gen": right_gen / ng,
            f"nna_{name}_ref": right_ref / nr, "n_gen": ng, "n_ref": nr}


def set_metrics_host(cd_gg, cd_gr, cd_rr, name="cd"):
    """The numpy statement of set_metrics (np.argmin returns the first minimum: the same lowest-index rule)."""
    import math
    import numpy as np
    gg, gr, rr = (np.asarray(m, dtype=np.float64) for m in (cd_gg, cd_gr, cd_rr))
    ng, nr = gr.shape
    union = np.block([[gg, gr], [gr.T, rr]])
    np.fill_diagonal(union, np.inf)
    nn = union.argmin(1)
    same = (nn >= ng) == (np.arange(ng + nr) >= ng)
    return {f"mmd_{name}": math.fsum(gr.min(0).tolist()) / nr, f"cov_{name}": len(set(gr.argmin(1).tolist())) / nr,
            f"nna_{name}": int(same.sum()) / (ng + nr), f"nna_{name}_gen": int(same[:ng].sum()) / ng,
            f"nna_{name}_ref": int(same[ng:].sum()) / nr, "n_gen": ng, "n_ref": nr}


def generation_metrics(gen, ref, emd=False, emd_eps=EMD_EPS):
    """MMD-CD / COV-CD / 1-NNA-CD (set_metrics) of a generated set against a reference set: lists of (n_i, >= 3) device
    tensors or padded (N, P, >= 3) tensors.  Three Chamfer matrices: gen x gen and ref x ref (symmetric), gen x ref.
    emd=True adds the same three under the Earth Mover's Distance (mmd_emd, cov_emd, nna_emd, nna_emd_gen, nna_emd_ref)
    from three emd_matrix calls; every cloud must then hold the same number of points, at most 2 048."""
    gs, rs = _clouds(gen, None, "gen"), _clouds(ref, None, "ref")
    if emd:
        _emd_sizes(gs + rs)
    out = set_metrics(chamfer_matrix(gs), chamfer_matrix(gs, rs), chamfer_matrix(rs))
    if emd:
        out.update(set_metrics(emd_matrix(gs, eps=emd_eps), emd_matrix(gs, rs, eps=emd_eps), emd_matrix(rs, eps=emd_eps),
                               name="emd"))
    return out


# ---- Earth Mover's Distance: epsilon-scaling auction (rangeldm_amd/csrc/emd.hip) ----------------------------------------
def _emd_sizes(clouds):
    """The common point count of the clouds; ValueError (before the device) if they differ or exceed the kernel's size."""
    sizes = sorted({int(c.shape[0]) for c in clouds})
    if len(sizes) != 1:
        raise ValueError(f"EMD is a one-to-one matching: every cloud must hold the same number of points, got clouds of "
                         f"{sizes[0]} and of {sizes[-1]} points (sub-sample them to a common size first)")
    if sizes[0] > EMD_MAX_POINTS:
        raise ValueError(f"EMD is a one-to-one matching held in one wave's registers: at most {EMD_MAX_POINTS} points per "
                         f"cloud, got {sizes[0]}")
    return sizes[0]


def _emd_eps(eps):
    import math
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"eps must be positive and finite, got {eps}")
    return eps


def _emd_status(rc, message, what="rldm_emd_matrix"):
    """Map rldm_emd_matrix's return value: 0 passes; RLDM_EMD_BID_CAP raises EmdBidCapError naming the pair; anything else is
    the library's ordinary error."""
    if rc == 0:
        return
    if rc == _lib.RLDM_EMD_BID_CAP:
        raise EmdBidCapError(f"{what}: {message} (non-finite or pathological input? a larger eps needs fewer bids)")
    raise RuntimeError(f"librangeldm_hip: {what} failed: {message}")


class EmdBidCapError(RuntimeError):
    """A pair of clouds reached the auction's bid cap (1024 bids per point); no partial value is returned."""


def _emd_call(xp, xo, xk, nx, yp, yo, yk, ny, mode, eps, n, extras):
    dev = xp.device
    out = torch.zeros((nx, ny), dtype=torch.float64, device=dev)
    asg = price = bids = None
    if extras:
        asg = torch.full((nx, ny, n), -1, dtype=torch.int32, device=dev)
        price = torch.zeros((nx, ny, n), dtype=torch.float32, device=dev)
        bids = torch.zeros((nx, ny), dtype=torch.int32, device=dev)
    L = _lib.lib()
    rc = L.rldm_emd_matrix(xp.data_ptr(), xo.data_ptr(), xk, nx, yp.data_ptr(), yo.data_ptr(), yk, ny, mode, eps,
                           out.data_ptr(), asg.data_ptr() if extras else None, price.data_ptr() if extras else None,
                           bids.data_ptr() if extras else None, _lib.stream_ptr(dev))
    if rc != 0:
        msg = L.rldm_last_error()
        _emd_status(rc, msg.decode() if msg else "unknown error")
    return out, asg, price, bids


def emd_matrix(x, y=None, eps=EMD_EPS, return_assignment=False, x_lengths=None, y_lengths=None):
    """EMD[i][j] = (1 / N) min over one-to-one matchings a of sum_q |x_i[q] - y_j[a(q)]| (Euclidean, xyz only) for EVERY
    cloud of x against every cloud of y, to within the auction's certificate: an fp64 device (nx, ny) tensor.  y=None is the
    symmetric case (j > i computed and mirrored, zero diagonal).  Inputs as chamfer_matrix takes them, but EMD is a one-to-one
    matching: every cloud must hold the same number of points N <= 2 048 (ValueError before the device otherwise).

    The matching is found by an epsilon-scaling forward auction that ends at `eps` (metres): the value exceeds the optimum
    by at most eps plus a few fp32 roundings, and the returned prices prove it.  Every step is a single
    correctly rounded fp32 operation and the mean a fixed-order fp64 sum, so an entry depends on its two clouds and eps
    alone: two calls, a block of rows, and the symmetric and rectangular calls agree bit for bit.

    return_assignment=True returns (emd, assignment int32 (nx, ny, N), prices fp32 (nx, ny, N), bids int32 (nx, ny));
    in the symmetric case the assignment and prices are filled for j > i only (-1 / 0 elsewhere).  A pair that reaches
    1024 N bids raises EmdBidCapError naming it."""
    xs = _clouds(x, x_lengths, "x")
    ys = None if y is None else _clouds(y, y_lengths, "y")
    if y is None and y_lengths is not None:
        raise ValueError("y_lengths without y")
    n = _emd_sizes(xs + (ys or []))
    eps = _emd_eps(eps)
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = (xp, xo, xk) if ys is None else _pack(ys)
    nx, ny = len(xs), len(xs if ys is None else ys)
    out, asg, price, bids = _emd_call(xp, xo, xk, nx, yp, yo, yk, ny, _lib.RLDM_EMD_SYMMETRIC if ys is None else
                                      _lib.RLDM_EMD_RECT, eps, n, return_assignment)
    return (out, asg, price, bids) if return_assignment else out


def emd_pairs(x, y, eps=EMD_EPS, x_lengths=None, y_lengths=None):
    """Per-pair EMD, x_i against y_i: an fp64 device tensor [n].  The same kernel as emd_matrix, run on the diagonal of the
    matrix layout: entry i equals emd_matrix(x, y)[i][i] bit for bit."""
    xs, ys = _clouds(x, x_lengths, "x"), _clouds(y, y_lengths, "y")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} x clouds against {len(ys)} y clouds")
    n = _emd_sizes(xs + ys)
    eps = _emd_eps(eps)
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    yp, yo, yk = _pack(ys)
    out, _, _, _ = _emd_call(xp, xo, xk, len(xs), yp, yo, yk, len(ys), _lib.RLDM_EMD_DIAGONAL, eps, n, False)
    return torch.diagonal(out).clone()


# ---- Frechet distance over dumped activations (rangeldm_amd/csrc/frechet.hip) -------------------------------------------
class FrechetConvergenceError(RuntimeError):
    """The Jacobi loop reached its sweep cap (60 sweeps) with rotations still being applied; no value is returned."""


def _frechet_status(rc, message, what):
    """Map the return value of rldm_singular_values_f64 / rldm_frechet_distance: 0 passes; the sweep cap raises
    FrechetConvergenceError, non-finite input ValueError; anything else is the library's ordinary error."""
    if rc == 0:
        return
    if rc == _lib.RLDM_FRECHET_SWEEP_CAP:
        raise FrechetConvergenceError(f"{what}: {message}")
    if rc == _lib.RLDM_FRECHET_NONFINITE:
        raise ValueError(f"{what}: {message}")
    raise RuntimeError(f"librangeldm_hip: {what} failed: {message}")


def _frechet_check(rc, what):
    if rc != 0:
        msg = _lib.lib().rldm_last_error()
        _frechet_status(rc, msg.decode() if msg else "unknown error", what)


def _require_matrix(m, name):
    """ValueError unless m is a non-empty 2-D float tensor (checked before the device and the library are looked at)."""
    if not torch.is_tensor(m) or m.dim() != 2 or m.shape[0] == 0 or m.shape[1] == 0:
        raise ValueError(f"{name} must be a non-empty 2-D tensor, got {tuple(m.shape) if torch.is_tensor(m) else type(m)}")
    if not m.is_floating_point():
        raise ValueError(f"{name} must hold floating-point values, got {m.dtype}")
    return m


def _on_device(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("activations and matrices must live on the GPU (rangeldm_amd has no CPU path)")
    return [t.detach().to(torch.float64).contiguous() for t in tensors]


def _activation_sets(x, y):
    x, y = _require_matrix(x, "x"), _require_matrix(y, "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x holds {x.shape[1]} values per sample, y {y.shape[1]}")
    if x.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError(f"a covariance needs at least 2 samples per set, got {x.shape[0]} and {y.shape[0]}")
    return x, y


def gram_f64(a, b):
    """a . b^T for (n1, d) and (n2, d) device tensors, in fp64 on the fp64 MFMA: an fp64 device (n1, n2) tensor.  K is walked
    in one fixed order without split-K, so an entry depends on its two rows alone (a block of rows computed on its own equals
    those rows of the whole product bit for bit); operands and sums that are exact in fp64 give the exact product."""
    a, b = _require_matrix(a, "a"), _require_matrix(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"a holds {a.shape[1]} values per row, b {b.shape[1]}")
    a, b = _on_device(a, b)
    _lib.require_gpu()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().rldm_gram_f64(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], out.data_ptr(),
                                        _lib.stream_ptr(a.device)), "rldm_gram_f64")
    return out


def singular_values(m, tol=None, max_sweeps=60, return_sweeps=False):
    """The singular values of a (rows, cols) device tensor, fp64, sorted descending: min(rows, cols) of them.  One-sided
    (Hestenes) Jacobi on the orientation with fewer columns, round-robin pair order, one launch per step.  A
    pair of columns is left alone once |a_p . a_q| <= tol |a_p| |a_q| (tol None: sqrt(column length) * 2^-52); the loop ends
    with the first sweep that rotates nothing.  return_sweeps=True returns (values, sweeps run).  Raises ValueError for
    NaN / inf entries and FrechetConvergenceError when max_sweeps sweeps all rotated."""
    m = _require_matrix(m, "m")
    if int(max_sweeps) < 1:
        raise ValueError(f"max_sweeps must be at least 1, got {max_sweeps}")
    (m,) = _on_device(m)
    _lib.require_gpu()
    sv = torch.empty(min(m.shape), dtype=torch.float64, device=m.device)
    sweeps = C.c_int(0)
    _frechet_check(_lib.lib().rldm_singular_values_f64(m.data_ptr(), m.shape[0], m.shape[1], 0.0 if tol is None else float(tol),
                                                       int(max_sweeps), sv.data_ptr(), C.byref(sweeps),
                                                       _lib.stream_ptr(m.device)), "rldm_singular_values_f64")
    return (sv, sweeps.value) if return_sweeps else sv


def frechet_distance(x, y, return_terms=False):
    """metrics/metrics/fid/fid_score.py calculate_frechet_distance(np.mean(x, 0), np.cov(x, rowvar=False), ... of y): the
    Frechet distance between the Gaussians fitted to two sets of activations, (n1, d) and (n2, d) device tensors of any float
    dtype (converted to fp64), n1, n2 >= 2.  No d x d matrix is formed: with A, B the centred sets,

        Tr sqrtm(C1 C2) = |A B^T|_* / sqrt((n1 - 1)(n2 - 1))         (nuclear norm: the sum of singular values)

    so the work is two column means, two sums of squares, one (n1, n2) Gram product over d and the singular values of that
    matrix.  Every reduction runs in a fixed order: two calls agree bit for bit.  The value is NOT clamped at 0 (the reference
    does not clamp): identical sets give a rounding-sized number of either sign.

    Returns the distance as a float; return_terms=True returns a dict: frd, mean_sq (|mu1 - mu2|^2), tr1, tr2 (Tr C1, Tr C2),
    tr_sqrt (Tr sqrtm(C1 C2)) and sweeps (Jacobi sweeps run); frd = mean_sq + tr1 + tr2 - 2 tr_sqrt.
    Raises ValueError for shapes that do not fit (before the device) and for NaN / inf activations, RuntimeError for host
    tensors, FrechetConvergenceError if the Jacobi loop reaches its cap of 60 sweeps."""
    x, y = _activation_sets(x, y)
    x, y = _on_device(x, y)
    _lib.require_gpu()
    out = (C.c_double * 5)()
    L = _lib.lib()
    _frechet_check(L.rldm_frechet_distance(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], x.shape[1], out,
                                           _lib.stream_ptr(x.device)), "rldm_frechet_distance")
    if not return_terms:
        return out[0]
    return {"frd": out[0], "mean_sq": out[1], "tr1": out[2], "tr2": out[3], "tr_sqrt": out[4],
            "sweeps": int(L.rldm_frechet_last_sweeps())}


def frechet_distance_host(x, y):
    """The numpy statement of frechet_distance, fp64: np.linalg.svd(A @ B.T, compute_uv=False).sum() for the trace term."""
    import numpy as np
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1] or x.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError(f"x and y must be (n >= 2, d) with the same d, got {x.shape} and {y.shape}")
    mu1, mu2 = x.mean(0), y.mean(0)
    a, b = x - mu1, y - mu2
    n1, n2 = x.shape[0], y.shape[0]
    diff = mu1 - mu2
    tr_sqrt = np.linalg.svd(a @ b.T, compute_uv=False).sum() / np.sqrt((n1 - 1.0) * (n2 - 1.0))
    return float(diff.dot(diff) + (a * a).sum() / (n1 - 1) + (b * b).sum() / (n2 - 1) - 2.0 * tr_sqrt)


FRD_TOTAL, FRD_COUNT, FRD_LIMIT = 2097152, 4096, 1100     # values per dumped file, values kept, files used per folder


def frd_indices(total=FRD_TOTAL, count=FRD_COUNT, seed=0):
    """metrics/metrics/fid/lidargen_fid.py get_fid's draw: `random.seed(seed); random.sample(range(total), count)`."""
    import random
    return random.Random(seed).sample(range(total), count)


def load_activations(folder, indices, limit=FRD_LIMIT, total=FRD_TOTAL, device="cuda"):
    """lidargen_fid.py load_activations: `np.load(f).reshape(-1)[indices]` of the `.npy` files of `folder`, stacked into a
    (files, len(indices)) tensor on `device` in the files' dtype.  At most `limit` files are used, taken in SORTED order: the
    reference takes them in glob order and then `[0:1100]`, which is an arbitrary subset once a folder holds more than 1 100
    files; sorted order makes the choice a function of the names.  A file whose flattened size is not `total` raises
    ValueError naming it."""
    import glob
    import os
    import numpy as np
    files = sorted(glob.glob(os.path.join(folder, "*.npy")))[:limit]
    if not files:
        raise FileNotFoundError(f"no .npy files in {folder}")
    idx = np.asarray(indices, dtype=np.int64)
    rows = []
    for path in files:
        flat = np.load(path).reshape(-1)
        if flat.shape[0] != total:
            raise ValueError(f"{path}: {flat.shape[0]} values, expected {total}")
        rows.append(flat[idx])
    return torch.from_numpy(np.stack(rows, 0)).to(device)


# ---- kernel distance and precision / recall / density / coverage (rangeldm_amd/csrc/feature_metrics.hip) -----------------
FEATURE_K_CAP = 16          # RLDM_FEATURE_MAX_K: a row keeps its k + 1 smallest squared distances for k up to this

FeatureScan = collections.namedtuple("FeatureScan", "kmin_sq count_a count_b min_sq poly_sum")
FeatureScan.__doc__ = """The per-row outputs of feature_scan / feature_scan_host; what was not asked for is None."""


def feature_scan_column_chunk(n_b):
    """Rows of b per column chunk of feature_scan: 64 * ceil(ceil(n_b / 64) / 16), a function of n_b alone (at most 16
    chunks).  poly_sum is the sum, over ascending chunks, of each chunk's sum over ascending j."""
    return 64 * -(-(-(-int(n_b) // 64)) // 16)


def _scan_shapes(sa, sb, k, ra, rb, row_offset):
    """The ValueErrors of feature_scan / feature_scan_host, from shapes alone (a shape of None: not given)."""
    if len(sa) != 2 or len(sb) != 2 or 0 in sa or 0 in sb:
        raise ValueError(f"a and b must be non-empty 2-D, got {tuple(sa)} and {tuple(sb)}")
    if sa[1] != sb[1]:
        raise ValueError(f"a holds {sa[1]} values per row, b {sb[1]}")
    if k is not None:
        if int(k) != k or not 1 <= k <= FEATURE_K_CAP:
            raise ValueError(f"k must be an integer in [1, {FEATURE_K_CAP}], got {k}")
        if sb[0] < k + 1:
            raise ValueError(f"the k + 1 = {k + 1} smallest distances of a row need at least {k + 1} rows of b, got {sb[0]}")
    if ra is not None and tuple(ra) != (sa[0],):
        raise ValueError(f"radius_sq_a must hold one value per row of a ({sa[0]}), got shape {tuple(ra)}")
    if rb is not None and tuple(rb) != (sb[0],):
        raise ValueError(f"radius_sq_b must hold one value per row of b ({sb[0]}), got shape {tuple(rb)}")
    if int(row_offset) != row_offset or row_offset < 0:
        raise ValueError(f"row_offset must be a non-negative integer, got {row_offset}")


def feature_scan(a, b, k=None, radius_sq_a=None, radius_sq_b=None, poly=False, exclude_diagonal=False, row_offset=0):
    """One scan of the rows of a (n_a, d) against the rows of b (n_b, d), device tensors of any float dtype (converted to
    fp64), folded into per-row outputs: a FeatureScan of device tensors.  No (n_a, n_b) matrix is formed; the workspace is
    O(n_a + n_b).  All arithmetic is fp64:

        g(x, y)   the dot product as gram_f64 computes it (K ascending in one fixed order, no split-K)
        s(x)      g(x, x), from the same product path
        d2(x, y)  max(0, (s(x) + s(y)) - 2 g(x, y)), in that order: identical rows are at exactly 0.  No square root is taken
        kappa     t = g(x, y) / d + 1; t * t * t          (the KID default: degree 3, gamma = 1 / d, coef0 = 1)

        kmin_sq   (n_a, k + 1)  the k + 1 smallest d2 of the row, ascending            (k given; k <= FEATURE_K_CAP, n_b >= k + 1)
        count_a   (n_a,) int32  #{j : d2 < radius_sq_a[row]}                          (radius_sq_a (n_a,) given)
        count_b   (n_a,) int32  #{j : d2 < radius_sq_b[j]}                            (radius_sq_b (n_b,) given)
        min_sq    (n_a,)        the smallest d2 of the row                            (always)
        poly_sum  (n_a,)        sum_j kappa, ascending j within a column chunk and ascending chunks
                                (feature_scan_column_chunk); with exclude_diagonal without j == row + row_offset   (poly)

    Comparisons are strict.  A row's outputs depend on that row, on b and on row_offset alone: feature_scan(a[3:9], b, ...,
    row_offset=3) equals rows 3 .. 8 of the whole scan bit for bit, and two calls agree bit for bit.  Raises ValueError for
    arguments that do not fit (before the device is looked at) and for NaN / inf, RuntimeError for host tensors."""
    a, b = _require_matrix(a, "a"), _require_matrix(b, "b")
    for r in (radius_sq_a, radius_sq_b):
        if r is not None and (not torch.is_tensor(r) or not r.is_floating_point()):
            raise ValueError("a radius must be a floating-point tensor")
    _scan_shapes(a.shape, b.shape, k, None if radius_sq_a is None else radius_sq_a.shape,
                 None if radius_sq_b is None else radius_sq_b.shape, row_offset)
    a, b = _on_device(a, b)
    ra = None if radius_sq_a is None else _on_device(radius_sq_a)[0]
    rb = None if radius_sq_b is None else _on_device(radius_sq_b)[0]
    _lib.require_gpu()
    n_a, n_b, dev = a.shape[0], b.shape[0], a.device
    k1 = 0 if k is None else int(k) + 1
    f64 = dict(dtype=torch.float64, device=dev)
    out = FeatureScan(kmin_sq=torch.empty((n_a, k1), **f64) if k1 else None,
                      count_a=torch.empty(n_a, dtype=torch.int32, device=dev) if ra is not None else None,
                      count_b=torch.empty(n_a, dtype=torch.int32, device=dev) if rb is not None else None,
                      min_sq=torch.empty(n_a, **f64), poly_sum=torch.empty(n_a, **f64) if poly else None)
    ptr = lambda t: None if t is None else t.data_ptr()
    _frechet_check(_lib.lib().rldm_feature_scan_f64(a.data_ptr(), n_a, b.data_ptr(), n_b, a.shape[1], k1, ptr(ra), ptr(rb),
                                                    1 if poly else 0, 1 if exclude_diagonal else 0, int(row_offset),
                                                    ptr(out.kmin_sq), ptr(out.count_a), ptr(out.count_b), ptr(out.min_sq),
                                                    ptr(out.poly_sum), _lib.stream_ptr(dev)), "rldm_feature_scan_f64")
    return out


def feature_scan_host(a, b, k=None, radius_sq_a=None, radius_sq_b=None, poly=False, exclude_diagonal=False, row_offset=0):
    """The numpy statement of feature_scan (numpy arrays in, a FeatureScan of numpy arrays out): g = a @ b.T in fp64, s the
    rows' sums of squares, np.sort for the smallest values, np.cumsum (one add after the other) for poly_sum within a column
    chunk and the chunks added in ascending order.  Equal to the device bit for bit wherever the fp64 arithmetic is exact."""
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ra = None if radius_sq_a is None else np.asarray(radius_sq_a, dtype=np.float64)
    rb = None if radius_sq_b is None else np.asarray(radius_sq_b, dtype=np.float64)
    _scan_shapes(a.shape, b.shape, k, None if ra is None else ra.shape, None if rb is None else rb.shape, row_offset)
    g = a @ b.T
    s_a, s_b = np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", b, b)
    return _scan_fold_host(g, s_a, s_b, a.shape[1], k, ra, rb, poly, exclude_diagonal, row_offset)


def _scan_fold_host(g, s_a, s_b, d, k, ra, rb, poly, exclude_diagonal, row_offset):
    """The fold of feature_scan_host over given products g (n_a, n_b) and row norms s_a, s_b of d-term rows: everything
    after the dot products.  On gram_f64's own values it is what feature_scan returns, bit for bit."""
    import numpy as np
    n_a, n_b = g.shape
    d2 = np.maximum(0.0, (s_a[:, None] + s_b[None, :]) - 2.0 * g)
    poly_sum = None
    if poly:
        t = g / float(d) + 1.0
        kappa = t * t * t
        if exclude_diagonal:
            rows = np.arange(n_a) + int(row_offset)
            inside = rows < n_b
            kappa[np.nonzero(inside)[0], rows[inside]] = 0.0             # x + 0.0 is x: the same as skipping it
        chunk = feature_scan_column_chunk(n_b)
        poly_sum = np.zeros(n_a)
        for c0 in range(0, n_b, chunk):
            poly_sum = poly_sum + np.cumsum(kappa[:, c0:c0 + chunk], axis=1)[:, -1]
    return FeatureScan(kmin_sq=np.sort(d2, axis=1)[:, :k + 1] if k is not None else None,
                       count_a=(d2 < ra[:, None]).sum(1).astype(np.int32) if ra is not None else None,
                       count_b=(d2 < rb[None, :]).sum(1).astype(np.int32) if rb is not None else None,
                       min_sq=d2.min(1), poly_sum=poly_sum)


def knn_radii_sq(x, k=5):
    """r2_k(i): the (k + 1)-th smallest squared distance from row i of x to the rows of x, itself included (`prdc`'s
    get_kth_value(..., nearest_k + 1), squared): feature_scan(x, x, k=k).kmin_sq[:, k]."""
    return feature_scan(x, x, k=k).kmin_sq[:, k]


def _prdc_shapes(sr, sf, k):
    _scan_shapes(sr, sf, None, None, None, 0)
    if int(k) != k or not 1 <= k <= FEATURE_K_CAP:
        raise ValueError(f"k must be an integer in [1, {FEATURE_K_CAP}], got {k}")
    if min(sr[0], sf[0]) < k + 1:
        raise ValueError(f"a k = {k} neighbourhood needs at least {k + 1} rows per set, got {sr[0]} and {sf[0]}")


def _prdc_scores(scan, to_host, real, fake, k, return_terms):
    """The four scans and the four scores, for the device (scan = feature_scan) and the host statement alike."""
    n, m = real.shape[0], fake.shape[0]
    r_real = scan(real, real, k=k).kmin_sq[:, k]
    r_fake = scan(fake, fake, k=k).kmin_sq[:, k]
    by_real = scan(real, fake, radius_sq_a=r_real, radius_sq_b=r_fake)           # rows R against F
    by_fake = scan(fake, real, radius_sq_b=r_real)                               # rows F against R
    covered = by_real.min_sq < r_real
    counts = {"precision_count": int(to_host(by_fake.count_b > 0).sum()), "recall_count": int(to_host(by_real.count_b > 0).sum()),
              "density_count": int(to_host(by_fake.count_b).astype("int64").sum()), "coverage_count": int(to_host(covered).sum())}
    out = {"precision": counts["precision_count"] / m, "recall": counts["recall_count"] / n,
           "density": counts["density_count"] / (k * m), "coverage": counts["coverage_count"] / n}
    if return_terms:
        out.update(counts, radius_sq_real=r_real, radius_sq_fake=r_fake)
    return out


def prdc(real, fake, k=5, return_terms=False):
    """Precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020; the definitions of their
    `prdc` package) of the generated set `fake` (M, d) against the real set `real` (N, d) on k-nearest-neighbour manifolds:
    device tensors of any float dtype, N, M >= k + 1, 1 <= k <= FEATURE_K_CAP.  With d2 and r2_k as feature_scan and
    knn_radii_sq define them (squared distances throughout, strict <):

        precision = #{j : exists i, d2(R_i, F_j) < r2_k(R_i)} / M          recall   = #{i : exists j, d2(R_i, F_j) < r2_k(F_j)} / N
        density   = sum_j #{i : d2(R_i, F_j) < r2_k(R_i)} / (k M)          coverage = #{i : min_j d2(R_i, F_j) < r2_k(R_i)} / N

    Four scans (R.R, F.F, rows R against F, rows F against R), no (N, M) matrix; the counts are integers and each score is
    one division of two Python ints.  Returns a dict of the four scores; return_terms=True adds precision_count,
    recall_count, density_count, coverage_count and the radius vectors radius_sq_real, radius_sq_fake.  Raises ValueError
    for arguments that do not fit (before the device is looked at) and for NaN / inf, RuntimeError for host tensors."""
    real, fake = _require_matrix(real, "real"), _require_matrix(fake, "fake")
    _prdc_shapes(real.shape, fake.shape, k)
    real, fake = _on_device(real, fake)
    return _prdc_scores(feature_scan, lambda t: t.cpu().numpy(), real, fake, int(k), return_terms)


def prdc_host(real, fake, k=5, return_terms=False):
    """The numpy statement of prdc (feature_scan_host underneath)."""
    import numpy as np
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    _prdc_shapes(real.shape, fake.shape, k)
    return _prdc_scores(feature_scan_host, np.asarray, real, fake, int(k), return_terms)


def _subset_args(n, m, subsets):
    if int(subsets) != subsets or subsets < 1:
        raise ValueError(f"subsets must be a positive integer, got {subsets}")
    if int(m) != m or m < 2:
        raise ValueError(f"subset_size must be an integer of at least 2, got {m}")
    if m > n:
        raise ValueError(f"subset_size {m} rows cannot be drawn from {n}")


def kernel_subsets(n, m, subsets, seed, which):
    """The rows of the `subsets` subset estimates of kernel_distance: estimate s uses
    `random.Random(seed + 2 * s + which).sample(range(n), m)`, which = 0 for x and 1 for y (frd_indices' generator)."""
    import random
    if which not in (0, 1):
        raise ValueError(f"which must be 0 (x) or 1 (y), got {which}")
    _subset_args(n, m, subsets)
    return [random.Random(int(seed) + 2 * s + which).sample(range(int(n)), int(m)) for s in range(int(subsets))]


def _krd_shapes(sx, sy, subset_size, subsets):
    _scan_shapes(sx, sy, None, None, None, 0)
    if sx[0] < 2 or sy[0] < 2:
        raise ValueError(f"the unbiased estimate needs at least 2 rows per set, got {sx[0]} and {sy[0]}")
    if subset_size is not None:
        _subset_args(min(sx[0], sy[0]), subset_size, subsets)


def _krd_value(scan, to_list, x, y):
    import math
    n1, n2 = x.shape[0], y.shape[0]
    sxx = math.fsum(to_list(scan(x, x, poly=True, exclude_diagonal=True).poly_sum))
    syy = math.fsum(to_list(scan(y, y, poly=True, exclude_diagonal=True).poly_sum))
    sxy = math.fsum(to_list(scan(x, y, poly=True).poly_sum))
    return sxx / (n1 * (n1 - 1)) + syy / (n2 * (n2 - 1)) - (2.0 * sxy) / (n1 * n2), (sxx, syy, sxy)


def _krd(scan, to_list, take, x, y, subset_size, subsets, seed, return_terms):
    import math
    if subset_size is None:
        krd, (sxx, syy, sxy) = _krd_value(scan, to_list, x, y)
        return {"krd": krd, "sum_xx": sxx, "sum_yy": syy, "sum_xy": sxy} if return_terms else krd
    rows_x = kernel_subsets(x.shape[0], subset_size, subsets, seed, 0)
    rows_y = kernel_subsets(y.shape[0], subset_size, subsets, seed, 1)
    estimates = [_krd_value(scan, to_list, take(x, ix), take(y, iy))[0] for ix, iy in zip(rows_x, rows_y)]
    mean = math.fsum(estimates) / len(estimates)
    std = math.sqrt(math.fsum((e - mean) ** 2 for e in estimates) / len(estimates))
    out = {"krd": mean, "krd_std": std}
    if return_terms:
        out.update(estimates=estimates, subsets=int(subsets), subset_size=int(subset_size))
    return out


def kernel_distance(x, y, subset_size=None, subsets=100, seed=0, return_terms=False):
    """KRD: KID's unbiased estimate of the squared MMD (Binkowski et al. 2018) with the polynomial kernel
    kappa(a, b) = (g(a, b) / d + 1)^3 between two sets of activations, (n1, d) and (n2, d) device tensors of any float dtype,
    n1, n2 >= 2:

        KRD = sum_{i != j} kappa(x_i, x_j) / (n1 (n1 - 1)) + sum_{i != j} kappa(y_i, y_j) / (n2 (n2 - 1))
              - 2 sum_{i, j} kappa(x_i, y_j) / (n1 n2)

    Three scans (feature_scan(poly=True): per-row sums over ascending j, the diagonal skipped in the self terms), no (n1, n2)
    matrix; the three totals are math.fsum of the row sums, so they do not depend on how rows were batched.  Unlike the
    Frechet distance the estimate has no bias that depends on n.  The value is not clamped at 0.

    subset_size=None: the full-set estimate, a float (return_terms=True: a dict krd, sum_xx, sum_yy, sum_xy).
    subset_size=m: a dict krd (the mean) and krd_std (the population standard deviation) over `subsets` estimates, estimate s
    on the rows kernel_subsets(n1, m, subsets, seed, 0)[s] of x and kernel_subsets(n2, m, subsets, seed, 1)[s] of y;
    return_terms=True adds estimates, subsets and subset_size.
    Raises ValueError for arguments that do not fit (before the device is looked at) and for NaN / inf, RuntimeError for host
    tensors."""
    x, y = _require_matrix(x, "x"), _require_matrix(y, "y")
    _krd_shapes(x.shape, y.shape, subset_size, subsets)
    x, y = _on_device(x, y)
    take = lambda t, rows: t[torch.as_tensor(rows, device=t.device)]
    return _krd(feature_scan, lambda t: t.cpu().tolist(), take, x, y, subset_size, subsets, seed, return_terms)


def kernel_distance_host(x, y, subset_size=None, subsets=100, seed=0, return_terms=False):
    """The numpy statement of kernel_distance (feature_scan_host underneath)."""
    import numpy as np
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    _krd_shapes(x.shape, y.shape, subset_size, subsets)
    return _krd(feature_scan_host, lambda t: t.tolist(), lambda t, rows: t[np.asarray(rows)], x, y, subset_size, subsets, seed,
                return_terms)


def farthest_point_sample(x, k, x_lengths=None, start=0):
    """Farthest point sampling of every cloud: an int64 device tensor (B, k) of indices into each cloud, in selection order.
    Inputs as chamfer_matrix takes them (a list of (P_i, >= 3) device tensors, or a padded tensor plus lengths); only xyz is
    read.  `start` (an int, or one per cloud) is the first selected index.  Per cloud, in fp32, one rounding per operation:

        mind = +inf everywhere; sel = start; k times: emit sel; d = ((dx*dx + dy*dy) + dz*dz), dx = x[i] - x[sel];
        mind = min(mind, d); mind[sel] = -inf; sel = the LOWEST index attaining max(mind)

    The -inf sentinel keeps a selected index out of every later round, so the k indices are distinct even on a cloud of
    duplicates.  A row depends on its cloud, k and start alone and equals the sequential numpy evaluation exactly; the
    indices for k are the first k of those for a larger k.  Raises ValueError (before the device) for k > P_i -- naming the
    cloud --, a start outside its cloud, clouds above FPS_MAX_POINTS points, and non-finite coordinates: min / arg-max over NaN
    is not a defined order."""
    xs = _clouds(x, x_lengths, "x")
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    starts = [int(start)] * len(xs) if not hasattr(start, "__len__") else [int(v) for v in start]
    if len(starts) != len(xs):
        raise ValueError(f"{len(starts)} start indices for {len(xs)} clouds")
    for i, (c, s0) in enumerate(zip(xs, starts)):
        p = int(c.shape[0])
        if k > p:
            raise ValueError(f"cloud {i} holds {p} points, fewer than k = {k}")
        if p > FPS_MAX_POINTS:
            raise ValueError(f"cloud {i} holds {p} points, above the {FPS_MAX_POINTS} farthest_point_sample takes")
        if not 0 <= s0 < p:
            raise ValueError(f"start {s0} is not an index of cloud {i} ({p} points)")
    finite = torch.stack([torch.isfinite(c[:, :3]).all() for c in xs]).tolist()          # (one read-back for the batch)
    if not all(finite):
        raise ValueError(f"cloud {finite.index(False)} holds non-finite coordinates (farthest point sampling orders distances)")
    _lib.require_gpu()
    xp, xo, xk = _pack(xs)
    first = torch.tensor(starts, dtype=torch.int32).to(xp.device)
    idx = torch.empty((len(xs), k), dtype=torch.int32, device=xp.device)
    _lib.check(_lib.lib().rldm_farthest_point_sample(xp.data_ptr(), xo.data_ptr(), xk, len(xs), k, first.data_ptr(),
                                                     idx.data_ptr(), _lib.stream_ptr(xp.device)), "rldm_farthest_point_sample")
    return idx.long()


SUBSAMPLE_METHODS = ("random", "fps")


def _fps_start(p, seed):
    import numpy as np
    return int(np.random.Generator(np.random.PCG64(int(seed))).integers(p))


def subsample(cloud, n, seed, method="random"):
    """`n` points of a (P, k) cloud chosen without replacement, in their original order; all of them if P <= n.  The choice
    is a function of (P, n, seed) alone (numpy's PCG64 on the host), so two runs and two rank counts pick the same points.
    method="fps" chooses by farthest point sampling instead (farthest_point_sample, started at the index
    `np.random.Generator(np.random.PCG64(seed)).integers(P)`): a function of the cloud, n and seed."""
    import numpy as np
    if method not in SUBSAMPLE_METHODS:
        raise ValueError(f"method must be one of {SUBSAMPLE_METHODS}, got {method!r}")
    P = int(cloud.shape[0])
    n = int(n)
    if n <= 0:
        raise ValueError(f"n must be positive, got {n}")
    if P <= n:
        return cloud
    if method == "fps":
        return subsample_batch([cloud], n, [seed], "fps")[0]
    idx = np.sort(np.random.Generator(np.random.PCG64(int(seed))).choice(P, size=n, replace=False))
    return cloud[torch.from_numpy(idx).to(cloud.device)]


def subsample_batch(clouds, n, seeds, method="random"):
    """[subsample(c, n, s, method) for c, s in zip(clouds, seeds)]; with method="fps" every cloud above n points goes
    through ONE farthest_point_sample call (one kernel launch for the ragged batch)."""
    if method not in SUBSAMPLE_METHODS:
        raise ValueError(f"method must be one of {SUBSAMPLE_METHODS}, got {method!r}")
    clouds, seeds = list(clouds), list(seeds)
    if len(clouds) != len(seeds):
        raise ValueError(f"{len(seeds)} seeds for {len(clouds)} clouds")
    n = int(n)
    if n <= 0:
        raise ValueError(f"n must be positive, got {n}")
    if method == "random":
        return [subsample(c, n, s) for c, s in zip(clouds, seeds)]
    out = list(clouds)
    large = [i for i, c in enumerate(clouds) if int(c.shape[0]) > n]
    if large:
        idx = farthest_point_sample([clouds[i] for i in large], n,
                                    start=[_fps_start(clouds[i].shape[0], seeds[i]) for i in large])
        idx = idx.sort(dim=1).values
        for row, i in zip(idx, large):
            out[i] = clouds[i][row.to(clouds[i].device)]
    return out


def range_errors(a, b, scale, shift=None, channels=None, window=None):
    """Per image fp64 (sum |a' - b'|, sum (a' - b')^2, pixel count) with v' = v * scale[c] + shift[c] (computed in fp64)
    over `channels` (default: all) and the azimuth columns [w0, w1) of `window` (default: all W; w1 may exceed W, the window
    then wraps past the seam).  a, b: (B, C, W, H) device fp32.  Returns (abs_sum (B,) fp64, sq_sum (B,) fp64, count)."""
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"a and b must be the same (B, C, W, H) shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, Cc, W, H = a.shape
    channels = list(range(Cc)) if channels is None else sorted(set(int(c) for c in channels))
    w0, w1 = (0, W) if window is None else (int(window[0]), int(window[1]))
    sc = (C.c_float * Cc)(*[float(v) for v in (scale if hasattr(scale, "__len__") else [scale] * Cc)])
    sh = (C.c_float * Cc)(*[float(v) for v in (shift if shift is not None else [0.0] * Cc)])
    if not a.is_cuda or not b.is_cuda:
        raise RuntimeError("range images must live on the GPU (rangeldm_amd has no CPU path)")
    a = a.detach().float().contiguous()
    b = b.detach().float().contiguous()
    mask = sum(1 << c for c in channels)
    sa = torch.empty(B, dtype=torch.float64, device=a.device)
    ss = torch.empty(B, dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().rldm_range_errors(a.data_ptr(), b.data_ptr(), B, Cc, W, H, mask, sc, sh, w0, w1, sa.data_ptr(),
                                            ss.data_ptr(), _lib.stream_ptr(a.device)), "rldm_range_errors")
    return sa, ss, len(channels) * (w1 - w0) * H


def cubic_weights(frac):
    """The four fp32 weights of OpenCV's `interpolateCubic` (Keys, A = -0.75) at fraction(s) `frac`, numpy, in its
    operation order -- the host statement of what beam_upsample(mode="bicubic") computes per output row."""
    import numpy as np
    x = np.asarray(frac, dtype=np.float32)
    A, one = np.float32(-0.75), np.float32(1.0)
    c0 = ((A * (x + one) - np.float32(5.0) * A) * (x + one) + np.float32(8.0) * A) * (x + one) - np.float32(4.0) * A
    c1 = ((A + np.float32(2.0)) * x - (A + np.float32(3.0))) * x * x + one
    c2 = ((A + np.float32(2.0)) * (one - x) - (A + np.float32(3.0))) * (one - x) * (one - x) + one
    c3 = one - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], -1).astype(np.float32)


def beam_upsample(images, rate, mode="nearest"):
    """(B, C, W, Hs) device fp32 -> (B, C, W, Hs * rate) along the beam axis: the baselines of metrics/metrics/mae.py:61-81
    (`cv2.resize(target[::rate], (0, 0), fx=1.0, fy=rate, interpolation=...)`).
      nearest: cv2 INTER_NEAREST, source row floor(r / rate).
      bicubic: cv2 INTER_CUBIC as restated here -- src = (r + 0.5) / rate - 0.5 (in double, then fp32), Keys weights with
               A = -0.75 in fp32 as OpenCV's interpolateCubic computes them (cubic_weights), source rows clamped to
               [0, Hs - 1], sum ((w0 s0 + w1 s1) + w2 s2) + w3 s3.  OpenCV is not available to pin this against: it is a
               restatement of its documented algorithm, not a bit-for-bit reproduction of cv2's output."""
    if mode not in ("nearest", "bicubic"):
        raise ValueError(f"mode must be 'nearest' or 'bicubic', got {mode!r}")
    if images.dim() != 4:
        raise ValueError(f"images must be (B, C, W, Hs), got {tuple(images.shape)}")
    if not images.is_cuda:
        raise RuntimeError("images must live on the GPU (rangeldm_amd has no CPU path)")
    x = images.detach().float().contiguous()
    B, Cc, W, Hs = x.shape
    out = torch.empty((B, Cc, W, Hs * int(rate)), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().rldm_beam_upsample(x.data_ptr(), B, Cc, W, Hs, int(rate), 0 if mode == "nearest" else 1,
                                             out.data_ptr(), _lib.stream_ptr(x.device)), "rldm_beam_upsample")
    return out
