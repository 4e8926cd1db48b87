"""All-pairs Chamfer matrix and the lowest-index row argmin (rangeldm_amd/csrc/chamfer.hip: chamfer_matrix_kernel,
matrix_finish_kernel, row_argmin_kernel; rangeldm_amd.metrics.chamfer_matrix / row_argmin).

    xy[i][j] = mean over q in X_i of min over t in Y_j of d2(q, t)        yx[i][j] = mean over t in Y_j of min over q in X_i
    d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, one rounding per operation

CPU: argument errors are raised before the device is touched.
GPU: integer-grid clouds are bit-equal to numpy fp64 (every minimum and every partial sum is an exact integer, the division is
one correctly rounded operation on both sides); random clouds are within the bound of a fixed-order fp64 sum of the brute-force
minima; the matrix agrees with the pair path; two calls, row blocks and the symmetric route give the same bits; ties go to
the lowest index.

The bound (derived, not measured): an fp64 sum of n non-negative terms in any fixed order is within (n - 1) * 2^-53 relative of
the exact sum; the division adds 2^-53, the reference (math.fsum, then one division) 2 * 2^-53: below n * 2^-52 for n >= 2, and
for n = 1 both sides are the same single value.
"""
import math

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M

SIZES = (1, 777, 2048, 2049, 4097, 3 * 2048 + 5)


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


def _ref_matrices(xs, ys, upper_only=False):
    """(xy, yx) in numpy fp64: the brute-force minima summed with math.fsum and divided once."""
    xy = np.zeros((len(xs), len(ys)))
    yx = np.zeros((len(xs), len(ys)))
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            if upper_only and j <= i:
                continue
            xy[i, j] = math.fsum(_brute_nn(x, y).astype(np.float64).tolist()) / len(x)
            yx[i, j] = math.fsum(_brute_nn(y, x).astype(np.float64).tolist()) / len(y)
    if upper_only:                                      # xy[j][i] = yx[i][j], yx[j][i] = xy[i][j], zero diagonal
        iu = np.triu_indices(len(xs), 1)
        xy.T[iu], yx.T[iu] = yx[iu], xy[iu]
    return xy, yx


def _dev(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _int_cloud(rng, n, stride):
    return rng.integers(-64, 65, (n, stride)).astype(np.float32)


def _cloud(rng, n, stride, scale=30.0):
    return (rng.standard_normal((n, stride)) * scale).astype(np.float32)


def _within_bound(got, ref, n_avg):
    """|got - ref| <= n * 2^-52 * ref per entry; n_avg[i][j] = points of the cloud the entry averages over"""
    got = got.cpu().numpy()
    err, bound = np.abs(got - ref), n_avg * 2.0 ** -52 * ref
    print("max |got - ref| / ref:", float(np.max(err / np.maximum(ref, 1e-300))), "bound / ref at most:", float(n_avg.max() * 2.0 ** -52))
    return bool(np.all(err <= bound))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    good = torch.zeros((5, 3))
    with pytest.raises(ValueError, match="empty"):
        M.chamfer_matrix([good, torch.zeros((0, 3))])
    with pytest.raises(ValueError, match="empty"):
        M.chamfer_matrix([good], [good, torch.zeros((0, 4))])
    with pytest.raises(ValueError, match="empty"):
        M.chamfer_matrix(torch.zeros((2, 4, 3)), x_lengths=torch.tensor([4, 0]))
    with pytest.raises(ValueError, match="no point clouds"):
        M.chamfer_matrix([])
    with pytest.raises(ValueError, match="no point clouds"):
        M.chamfer_matrix([good], [])
    with pytest.raises(ValueError):
        M.chamfer_matrix([torch.zeros((5, 2))])            # xyz needed
    with pytest.raises(ValueError):
        M.chamfer_matrix([good], [torch.zeros((5, 2))])
    with pytest.raises(ValueError):
        M.chamfer_matrix([good], None, y_lengths=[5])
    with pytest.raises(ValueError):
        M.row_argmin(torch.zeros((0, 3), dtype=torch.float64))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("xs_stride,ys_stride", [(3, 3), (4, 5), (5, 4)])
def test_integer_grid_rectangular_is_bit_equal_to_numpy(xs_stride, ys_stride):
    rng = np.random.default_rng(100 + xs_stride * 10 + ys_stride)
    xs = [_int_cloud(rng, n, xs_stride) for n in SIZES]
    ys = [_int_cloud(rng, n, ys_stride) for n in (2049, 1, 3 * 2048 + 5, 777, 2048, 4097)]
    xy, yx = M.chamfer_matrix(_dev(xs), _dev(ys), return_directions=True)
    rxy, ryx = _ref_matrices(xs, ys)
    assert xy.dtype == torch.float64 and tuple(xy.shape) == (len(xs), len(ys))
    assert np.array_equal(_bits(xy), rxy.view(np.uint64))
    assert np.array_equal(_bits(yx), ryx.view(np.uint64))
    cd = M.chamfer_matrix(_dev(xs), _dev(ys))
    assert np.array_equal(_bits(cd), (rxy + ryx).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [3, 4, 5])
def test_integer_grid_symmetric_is_bit_equal_to_numpy(stride):
    rng = np.random.default_rng(200 + stride)
    xs = [_int_cloud(rng, n, stride) for n in SIZES]
    xy, yx = M.chamfer_matrix(_dev(xs), return_directions=True)
    rxy, ryx = _ref_matrices(xs, xs, upper_only=True)
    assert np.array_equal(_bits(xy), rxy.view(np.uint64))
    assert np.array_equal(_bits(yx), ryx.view(np.uint64))


@pytest.mark.gpu
def test_padded_tensor_with_lengths_is_the_same_set():
    rng = np.random.default_rng(5)
    xs = [_int_cloud(rng, n, 3) for n in (40, 2500, 7)]
    pad = torch.zeros((3, 2500, 3))
    for i, c in enumerate(xs):
        pad[i, :len(c)] = torch.from_numpy(c)
    a = M.chamfer_matrix(pad.cuda(), x_lengths=[40, 2500, 7])
    b = M.chamfer_matrix(_dev(xs))
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_random_clouds_within_the_summation_bound():
    rng = np.random.default_rng(31)
    xs = [_cloud(rng, n, 4) for n in SIZES]
    ys = [_cloud(rng, n, 3) for n in (4097, 777, 1, 3 * 2048 + 5, 2048, 2049)]
    xy, yx = M.chamfer_matrix(_dev(xs), _dev(ys), return_directions=True)
    rxy, ryx = _ref_matrices(xs, ys)
    nx = np.array([[len(x)] * len(ys) for x in xs], np.float64)
    ny = np.array([[len(y) for y in ys]] * len(xs), np.float64)
    assert _within_bound(xy, rxy, nx)
    assert _within_bound(yx, ryx, ny)
    # symmetric
    sxy, syx = M.chamfer_matrix(_dev(xs), return_directions=True)
    rxy, ryx = _ref_matrices(xs, xs, upper_only=True)
    assert _within_bound(sxy, rxy, nx)
    assert _within_bound(syx, ryx, nx.T)


@pytest.mark.gpu
def test_matrix_agrees_with_the_pair_path():
    rng = np.random.default_rng(57)
    xs = [_cloud(rng, n, 3) for n in (300, 2048, 5000, 1, 2600)]
    ys = [_cloud(rng, n, 4) for n in (2048, 17, 4100, 900, 2049, 1, 7000)]
    dx, dy = _dev(xs), _dev(ys)
    xy, yx = M.chamfer_matrix(dx, dy, return_directions=True)
    # every pair through rldm_chamfer_nn / rldm_chamfer_mean: each cloud once per partner
    px = [dx[i] for i in range(5) for _ in range(7)]
    py = [dy[j] for _ in range(5) for j in range(7)]
    xm, ym = M.chamfer_pairs(px, py)
    xm, ym = xm.view(5, 7).cpu().numpy(), ym.view(5, 7).cpu().numpy()
    nx = np.array([[len(x)] * 7 for x in xs], np.float64)
    ny = np.array([[len(y) for y in ys]] * 5, np.float64)
    assert _within_bound(xy, xm, nx)
    assert _within_bound(yx, ym, ny)


@pytest.mark.gpu
def test_two_calls_row_blocks_and_symmetric_route_give_the_same_bits():
    rng = np.random.default_rng(77)
    xs = _dev([_cloud(rng, n, 3) for n in (2048, 513, 4500, 1, 2049, 9000, 300)])
    ys = _dev([_cloud(rng, n, 3) for n in (1000, 2048, 6200, 2)])
    xy, yx = M.chamfer_matrix(xs, ys, return_directions=True)
    xy2, yx2 = M.chamfer_matrix(xs, ys, return_directions=True)
    assert torch.equal(xy, xy2) and torch.equal(yx, yx2)
    for block in (1, 2, len(xs)):
        for lo in range(0, len(xs), block):
            bxy, byx = M.chamfer_matrix(xs[lo:lo + block], ys, return_directions=True)
            assert torch.equal(bxy, xy[lo:lo + block]) and torch.equal(byx, yx[lo:lo + block]), (block, lo)
    # symmetric against the rectangular call on (X, X)
    sxy, syx = M.chamfer_matrix(xs, return_directions=True)
    clones = [c.clone() for c in xs]
    rxy, ryx = M.chamfer_matrix(xs, clones, return_directions=True)
    n = len(xs)
    off = ~torch.eye(n, dtype=torch.bool, device="cuda")
    assert torch.equal(sxy[off], rxy[off]) and torch.equal(syx[off], ryx[off])
    assert float(sxy.diagonal().abs().max()) == 0.0 and float(syx.diagonal().abs().max()) == 0.0
    assert float(rxy.diagonal().abs().max()) == 0.0 and float(ryx.diagonal().abs().max()) == 0.0
    cd = M.chamfer_matrix(xs)
    assert torch.equal(cd, cd.t())
    assert torch.equal(sxy, syx.t())
    # row blocks of the symmetric matrix, as the evaluate driver shares them out over ranks
    for lo in range(0, n, 3):
        assert torch.equal(M.chamfer_matrix(xs[lo:lo + 3], xs), cd[lo:lo + 3])


@pytest.mark.gpu
def test_row_argmin_lowest_index_wins():
    rng = np.random.default_rng(13)
    a, b, c = _cloud(rng, 700, 3), _cloud(rng, 900, 3), _cloud(rng, 2500, 3) + np.float32(1000.0)
    xs = _dev([a, b, b.copy(), c, b.copy()])             # clouds 1, 2 and 4 are bit-identical
    cd = M.chamfer_matrix(xs)
    assert torch.equal(cd[:, 1], cd[:, 2]) and torch.equal(cd[:, 1], cd[:, 4])
    mn, arg = M.row_argmin(cd)
    assert arg.dtype == torch.int32 and arg.cpu().tolist() == [0, 1, 1, 3, 1]      # the zero diagonal, else the first zero
    assert mn.cpu().tolist() == [0.0] * 5
    mn, arg = M.row_argmin(cd, exclude_diag=True)
    ref = cd.cpu().numpy().copy()
    np.fill_diagonal(ref, np.inf)
    assert arg.cpu().tolist() == ref.argmin(1).tolist()
    assert arg[1].item() == 2 and arg[2].item() == 1 and arg[4].item() == 1        # the copies, lowest index, never itself
    assert arg[0].item() == 1                                                      # a tie between 1, 2 and 4 (3 is far away)
    assert np.array_equal(mn.cpu().numpy(), ref.min(1))
    # a wide matrix with planted ties, against numpy's first-minimum rule; rows longer than one pass of the workgroup
    m = rng.integers(0, 50, (37, 1500)).astype(np.float64)
    mn, arg = M.row_argmin(torch.from_numpy(m).cuda())
    assert arg.cpu().tolist() == m.argmin(1).tolist() and np.array_equal(mn.cpu().numpy(), m.min(1))
    sq = rng.integers(0, 9, (300, 300)).astype(np.float64)
    np.fill_diagonal(sq, -1.0)                                                     # the diagonal would win every row
    mn, arg = M.row_argmin(torch.from_numpy(sq).cuda(), exclude_diag=True)
    np.fill_diagonal(sq, np.inf)
    assert arg.cpu().tolist() == sq.argmin(1).tolist() and np.array_equal(mn.cpu().numpy(), sq.min(1))
    mn, arg = M.row_argmin(torch.zeros((1, 1), dtype=torch.float64, device="cuda"), exclude_diag=True)
    assert arg.item() == -1 and mn.item() == math.inf
