"""CPU: the numpy restatements of the deterministic mode's sums (rangeldm_amd.train_ops.*_host; the orders are stated in
include/rangeldm_hip.h at rldm_train_deterministic).  They are sums -- within fp32 (fp64 for the two losses) rounding distance of an
exact sum -- and they encode an ORDER: permuting the partials of a crafted input changes the bits, as fp32 addition is not
associative.  tests/test_train_deterministic_gpu.py holds the kernels to them bit for bit."""
import numpy as np

from rangeldm_amd import train_ops as T

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def _rng(seed):
    return np.random.default_rng(seed)


def test_chan_stats_host_is_a_sum():
    x = (_rng(1).standard_normal((2, 23, 9, 12)) * 3 + 1).astype(np.float32)      # 207 pixels: a short last partial
    cs = T.chan_stats_host(x)
    assert cs.dtype == np.float32 and cs.shape == (2, 12, 2)
    x64 = x.reshape(2, -1, 12).astype(np.float64)
    n = x64.shape[1]
    # every addition rounds by at most EPS32 of the running magnitude: <= n roundings of <= EPS32 * sum |x|
    for k, ref, mag in ((0, x64.sum(1), np.abs(x64).sum(1)), (1, (x64 * x64).sum(1), (x64 * x64).sum(1))):
        assert np.all(np.abs(cs[..., k] - ref) <= (n + 1) * EPS32 * mag)
    # added to what cs holds
    pre = _rng(2).standard_normal((2, 12, 2)).astype(np.float32)
    assert np.array_equal(T.chan_stats_host(x, pre), pre + cs)


def test_colsum_host_is_a_sum():
    dy = _rng(3).standard_normal((3, 40, 8, 10)).astype(np.float32)               # 320 pixels: two slabs, the second short
    rows, total = T.colsum_host(dy)
    d64 = dy.reshape(3, -1, 10).astype(np.float64)
    n = d64.shape[1]
    assert np.all(np.abs(rows - d64.sum(1)) <= (n + 1) * EPS32 * np.abs(d64).sum(1))
    assert np.all(np.abs(total - d64.sum((0, 1))) <= (3 * n + 1) * EPS32 * np.abs(d64).sum((0, 1)))
    pre_r, pre_t = _rng(4).standard_normal((3, 10)).astype(np.float32), _rng(5).standard_normal(10).astype(np.float32)
    r2, t2 = T.colsum_host(dy, rows=pre_r, total=pre_t)
    assert np.array_equal(r2, pre_r + rows) and np.array_equal(t2, pre_t + total)


def test_mse_and_sqnorm_host_are_sums():
    pred = _rng(6).standard_normal((2, 32, 8, 4)).astype(np.float32)
    target = _rng(7).standard_normal((2, 4, 32, 8)).astype(np.float32)
    w = _rng(8).random(2).astype(np.float32)
    d = (pred - target.transpose(0, 2, 3, 1)).astype(np.float64)                  # (the difference is taken in fp32)
    for weight, ref in ((None, (d * d).mean()), (w, (w.astype(np.float64)[:, None, None, None] * d * d).mean())):
        got = T.mse_host(pred, target, weight)
        assert abs(got - ref) <= (d.size + 4) * EPS64 * abs(ref)
    g = _rng(9).standard_normal((1 << 20) + 3).astype(np.float32)
    ref = (g.astype(np.float64) ** 2).sum()
    assert abs(T.sqnorm_host(g) - ref) <= 64 * EPS64 * ref                         # (a tree: few roundings per element)
    assert T.sqnorm_host(np.zeros(0, np.float32)) == 0.0


def _crafted(npix, slab):
    """One channel whose slabs hold (2^24, 1, 1, ..., -2^24 ...): in fp32 the order of the additions decides the result."""
    x = np.zeros((1, npix, 4), np.float32)
    x[0, 0 * slab, :] = 2.0 ** 24          # partial 0
    x[0, 1 * slab, :] = 1.0                # partial 1
    x[0, 2 * slab, :] = 1.0                # partial 2
    x[0, 3 * slab, :] = -2.0 ** 24         # partial 3
    return x


def _permute_slabs(x, slab, order):
    B, npix, Cc = x.shape
    return x.reshape(B, npix // slab, slab, Cc)[:, order].reshape(B, npix, Cc)


def test_host_restatements_encode_the_fold_order():
    # the fold: (((2^24 + 1) + 1) - 2^24) = 0 in fp32 (each + 1 is lost), while ((1 + 1) + 2^24) - 2^24 = 2
    for slab, fn in ((64, lambda v: T.chan_stats_host(v)[0, 0, 0]), (256, lambda v: T.colsum_host(v)[0][0, 0])):
        x = _crafted(4 * slab, slab)
        assert fn(x) == 0.0
        assert fn(_permute_slabs(x, slab, [1, 2, 0, 3])) == 2.0
        assert fn(_permute_slabs(x, slab, [0, 3, 1, 2])) == 2.0
    # colsum's total: the image sums in image order
    dy = np.zeros((4, 16, 1), np.float32)
    dy[:, 0, 0] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]
    assert T.colsum_host(dy)[1][0] == 0.0 and T.colsum_host(dy[[1, 2, 0, 3]])[1][0] == 2.0


def test_host_restatements_encode_the_order_inside_a_partial():
    # lane k adds pixels k, k + 16, k + 32, k + 48 in that order, then the lanes are added k = 0 .. 15
    x = np.zeros((1, 64, 4), np.float32)
    x[0, [0, 16, 32, 48], 0] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]                  # all in lane 0: (((2^24 + 1) + 1) - 2^24) = 0
    assert T.chan_stats_host(x)[0, 0, 0] == 0.0
    y = np.zeros_like(x)
    y[0, [32, 0, 16, 48], 0] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]                  # the same values permuted inside the lane:
    assert T.chan_stats_host(y)[0, 0, 0] == 2.0                                   # ((1 + 1) + 2^24) - 2^24
    z = np.zeros_like(x)
    z[0, [0, 1, 2, 3], 0] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]                     # one value per lane: the lanes are folded in order
    assert T.chan_stats_host(z)[0, 0, 0] == 0.0
    z[0, [0, 1, 2, 3], 0] = [1.0, 1.0, 2.0 ** 24, -2.0 ** 24]
    assert T.chan_stats_host(z)[0, 0, 0] == 2.0
    # the square is rounded to fp32 BEFORE it is added (no fused multiply-add): 4097^2 = 2^24 + 8193 rounds to 2^24 + 8192
    s = np.zeros((1, 64, 4), np.float32)
    s[0, 0, 0], s[0, 16, 0] = 4097.0, 4097.0
    assert T.chan_stats_host(s)[0, 0, 1] == 2.0 * (2.0 ** 24 + 8192.0)


def test_double_folds_encode_an_order():
    # thread t adds partials t, t + 256, ... in order; then a fixed tree
    part = np.zeros(1024, np.float64)
    part[[0, 256, 512, 768]] = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]
    assert T._fold_double(part) == 0.0
    part[[0, 256, 512, 768]] = [1.0, 1.0, 2.0 ** 53, -2.0 ** 53]
    assert T._fold_double(part) == 2.0
    # the tree inside a block: lanes l and l ^ 32 meet first
    a = np.zeros((1, 256), np.float64)
    a[0, [0, 32, 1, 33]] = [2.0 ** 54, -2.0 ** 54, 1.0, 1.0]
    assert T._block_sum(a)[0] == 2.0
    a[:] = 0
    a[0, [0, 1, 32, 33]] = [2.0 ** 54, -2.0 ** 54, 1.0, 1.0]                      # (2^54 + 1) + (-2^54 + 1): both 1s are lost
    assert T._block_sum(a)[0] == 0.0
