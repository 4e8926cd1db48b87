"""Chamfer distance (rangeldm_amd/csrc/chamfer.hip; pytorch3d.loss.chamfer_distance as ldm/convert_vae.py:262-271 calls it).

CPU: argument checks that run before the device is touched (empty clouds are a ValueError).
GPU: every per-point nearest squared distance is BIT-EQUAL to a CPU fp32 brute force of ((dx*dx + dy*dy) + dz*dz) --
no FMA contraction and a min over exactly the same values, whatever the target split; integer-grid clouds give exact
integers; a KITTI-size pair matches a cKDTree fp64 reference to 1e-6; two calls are bit-identical.
"""
import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M


def _brute_nn(q, t):
    """min over t of ((dx*dx + dy*dy) + dz*dz) in fp32, numpy element-wise ops (one rounding each, no FMA)."""
    q = np.ascontiguousarray(q[:, :3], np.float32)
    t = np.ascontiguousarray(t[:, :3], np.float32)
    out = np.empty(len(q), np.float32)
    step = max(1, (1 << 22) // max(1, len(t)))
    for i in range(0, len(q), step):
        qq = q[i:i + step]
        dx = qq[:, None, 0] - t[None, :, 0]
        dy = qq[:, None, 1] - t[None, :, 1]
        dz = qq[:, None, 2] - t[None, :, 2]
        out[i:i + step] = ((dx * dx + dy * dy) + dz * dz).min(1)
    return out


def _cloud(rng, n, stride, scale=30.0):
    c = (rng.standard_normal((n, stride)) * scale).astype(np.float32)
    return c


def test_empty_cloud_is_a_value_error():
    good = torch.zeros((5, 3))
    with pytest.raises(ValueError, match="empty"):
        M.chamfer_distance([good, torch.zeros((0, 3))], [good, good])
    with pytest.raises(ValueError, match="empty"):
        M.chamfer_distance(torch.zeros((2, 4, 3)), torch.zeros((2, 4, 3)), x_lengths=torch.tensor([4, 0]))
    with pytest.raises(ValueError):
        M.nearest_sq_dists([], [])
    with pytest.raises(ValueError):
        M.chamfer_distance([good], [good, good])          # pairs must match
    with pytest.raises(ValueError):
        M.chamfer_distance([torch.zeros((5, 2))], [good])  # xyz needed


def _check_bit_equal(xs, ys):
    xn, yn = M.nearest_sq_dists([torch.from_numpy(x).cuda() for x in xs], [torch.from_numpy(y).cuda() for y in ys])
    for x, y, a, b in zip(xs, ys, xn, yn):
        ra, rb = _brute_nn(x, y), _brute_nn(y, x)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), ra.view(np.uint32)), (len(x), len(y))
        assert np.array_equal(b.cpu().numpy().view(np.uint32), rb.view(np.uint32)), (len(x), len(y))


@pytest.mark.gpu
@pytest.mark.parametrize("xs_stride,ys_stride", [(3, 3), (4, 5), (5, 4)])
def test_nn_bit_equal_mixed_sizes(xs_stride, ys_stride):
    rng = np.random.default_rng(7 + xs_stride * 10 + ys_stride)
    sizes = [(1, 1), (1, 777), (777, 1), (2049, 513), (4097, 3001), (300, 2048 * 3 + 5)]
    xs = [_cloud(rng, a, xs_stride) for a, _ in sizes]
    ys = [_cloud(rng, b, ys_stride) for _, b in sizes]
    dup = _cloud(rng, 600, xs_stride)
    dup[300:] = dup[:300]                                        # duplicate points inside one cloud
    xs.append(dup)
    ys.append(np.concatenate([dup[:200, :ys_stride] if ys_stride <= xs_stride else
                              np.pad(dup[:200], ((0, 0), (0, ys_stride - xs_stride))), _cloud(rng, 100, ys_stride)]))
    _check_bit_equal(xs, ys)


@pytest.mark.gpu
def test_identical_clouds_have_zero_distance():
    rng = np.random.default_rng(3)
    c = _cloud(rng, 5000, 4)
    x = torch.from_numpy(c).cuda()
    d, _ = M.chamfer_distance([x, x[:17]], [x.clone(), x[:17].clone()])
    assert float(d) == 0.0
    xn, yn = M.nearest_sq_dists([x], [x])
    assert float(xn[0].max()) == 0.0 and float(yn[0].max()) == 0.0


@pytest.mark.gpu
def test_one_pair_split_across_many_workgroups():
    # one pair alone: the targets are split over ~40 workgroups per query block, merged with atomicMin on the bits
    rng = np.random.default_rng(11)
    x, y = _cloud(rng, 3000, 3), _cloud(rng, 20000, 3)
    _check_bit_equal([x], [y])


@pytest.mark.gpu
def test_integer_grid_clouds_are_exact():
    rng = np.random.default_rng(5)
    xs = [rng.integers(-60, 61, (n, 3)).astype(np.float32) for n in (1000, 2500, 7)]
    ys = [rng.integers(-60, 61, (n, 3)).astype(np.float32) for n in (1300, 9, 4100)]
    xn, yn = M.nearest_sq_dists([torch.from_numpy(a).cuda() for a in xs], [torch.from_numpy(b).cuda() for b in ys])
    xm, ym = M.chamfer_pairs([torch.from_numpy(a).cuda() for a in xs], [torch.from_numpy(b).cuda() for b in ys])
    for i, (a, b) in enumerate(zip(xs, ys)):
        ai, bi = a.astype(np.int64), b.astype(np.int64)
        ra = ((ai[:, None, :] - bi[None, :, :]) ** 2).sum(-1).min(1)
        rb = ((bi[:, None, :] - ai[None, :, :]) ** 2).sum(-1).min(1)
        assert np.array_equal(xn[i].cpu().numpy(), ra.astype(np.float32))
        assert np.array_equal(yn[i].cpu().numpy(), rb.astype(np.float32))
        assert float(xm[i]) == ra.sum() / len(ra) and float(ym[i]) == rb.sum() / len(rb)


def _kitti_like(rng, n):
    r = rng.uniform(3.0, 70.0, n)
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.43, 0.03, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el) + 1.7], 1).astype(np.float32)


@pytest.mark.gpu
def test_kitti_size_pair_matches_kdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(2024)
    x, y = _kitti_like(rng, 65536), _kitti_like(rng, 60000)
    d, _ = M.chamfer_distance([torch.from_numpy(x).cuda()], [torch.from_numpy(y).cuda()])
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    dx, _ = cKDTree(y64).query(x64, k=1, workers=16)
    dy, _ = cKDTree(x64).query(y64, k=1, workers=16)
    ref = np.mean(dx ** 2) + np.mean(dy ** 2)
    assert abs(float(d) - ref) <= 1e-6 * ref, (float(d), ref)


@pytest.mark.gpu
def test_two_calls_are_bit_identical_and_reductions_agree():
    rng = np.random.default_rng(9)
    xs = [torch.from_numpy(_kitti_like(rng, n)).cuda() for n in (20000, 513, 4096)]
    ys = [torch.from_numpy(_kitti_like(rng, n)).cuda() for n in (18000, 7000, 1)]
    a1, b1 = M.nearest_sq_dists(xs, ys)
    a2, b2 = M.nearest_sq_dists(xs, ys)
    for u, v in zip(a1 + b1, a2 + b2):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    xm1, ym1 = M.chamfer_pairs(xs, ys)
    xm2, ym2 = M.chamfer_pairs(xs, ys)
    assert torch.equal(xm1, xm2) and torch.equal(ym1, ym2)
    # the per-pair means are the fp64 means of the per-point minima
    for i in range(3):
        assert abs(float(xm1[i]) - a1[i].double().mean().item()) <= 1e-12 * float(xm1[i])
        assert abs(float(ym1[i]) - b1[i].double().mean().item()) <= 1e-12 * max(float(ym1[i]), 1e-30)
    # pytorch3d's reduction: mean over pairs of the per-pair sums; padded + lengths gives the same pairs
    d, none = M.chamfer_distance(xs, ys)
    assert none is None and float(d) == float((xm1 + ym1).mean())
    P = max(t.shape[0] for t in xs)
    pad = torch.zeros((3, P, 3), device="cuda")
    for i, t in enumerate(xs):
        pad[i, :t.shape[0]] = t
    Q = max(t.shape[0] for t in ys)
    pady = torch.zeros((3, Q, 3), device="cuda")
    for i, t in enumerate(ys):
        pady[i, :t.shape[0]] = t
    dp, _ = M.chamfer_distance(pad, pady, x_lengths=torch.tensor([t.shape[0] for t in xs]),
                               y_lengths=[t.shape[0] for t in ys])
    assert float(dp) == float(d)
    per, _ = M.chamfer_distance(xs, ys, batch_reduction=None)
    assert torch.equal(per, xm1 + ym1)
