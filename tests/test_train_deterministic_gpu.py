"""GPU: the deterministic mode of the training step (rldm_train_deterministic, UNetTrainer(deterministic=True)).

1. every op repeats bit for bit, alone and beside a large device-to-device copy on a second stream (which shifts workgroup arrival);
2. nothing is lost or counted twice: integer-valued operands (tests/test_train_exact.py's grid) give the fp64 reference exactly;
3. the order stated in include/rangeldm_hip.h is the order: the numpy restatements of train_ops agree bit for bit, and the statistics
   a fused conv accumulates for its output equal chan_stats of the stored output;
4. / 5. whole steps, small and fused, repeat bit for bit; the deterministic gradients stay inside the run-to-run gate of
   tests/test_training.py against the default mode;
6. the switch is scoped to the trainer's calls.

Shapes: the smallest that reach each code path (asserted where the path depends on the shape).  One deviation from the issue's list:
`rldm_train_conv_splits` is 1 for the 1x1 conv with Cin = 64 (conv_lds_plan never splits fewer than three stages), so that case
is kept as the unsplit 1x1 and a 1x1 with Cin = 512, which does split, is added beside it.  Likewise the 256 x 16, 64 -> 64 fused conv
at B = 2 has 128 workgroups and is split in the default mode; in the deterministic mode it runs unsplit with 64 tiles per image, which
is what the case is there for.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from rangeldm_amd.config import UNetConfig
from rangeldm_amd.params import unet_param_shapes
from rangeldm_amd.synth import synth_state_dict
from oracle import ops as o_ops
from tests.hip_util import amax, assert_bitexact, assert_exact_bound, int_grid, silu_targets

pytestmark = pytest.mark.gpu
SMALL = dict(sample_size=(32, 8), block_out_channels=(32, 32, 64, 64))
U = 2.0 ** -5


def _T():
    from rangeldm_amd import train_ops as T
    return T


@contextlib.contextmanager
def det(on=True):
    T = _T()
    prev = T.deterministic_enabled()
    T.deterministic(on)
    try:
        yield
    finally:
        T.deterministic(prev)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


_side = {}


def repeats_exactly(fn, what):
    """fn() -> tuple of tensors, ten times on the same inputs in the deterministic mode: five alone, five while a second stream copies
    256 MB device to device.  All ten equal as bit patterns."""
    if not _side:
        _side["a"] = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        _side["b"] = torch.empty_like(_side["a"])
        _side["s"] = torch.cuda.Stream()
    first = None
    with det():
        for i in range(10):
            torch.cuda.synchronize()
            if i >= 5:
                with torch.cuda.stream(_side["s"]):
                    _side["b"].copy_(_side["a"], non_blocking=True)
            out = fn()
            out = out if isinstance(out, (tuple, list)) else (out,)
            got = [bits(t) for t in out]
            torch.cuda.synchronize()
            if first is None:
                first = got
                continue
            for k, (a, b) in enumerate(zip(first, got)):
                assert torch.equal(a, b), f"{what}: output {k} of run {i} differs from run 0 in {int((a != b).sum())} elements"


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def splits(x, N, taps, stride=1, mode=0):
    from rangeldm_amd import _lib
    T = _T()
    d = T.conv_desc(x, N, taps, stride, mode)
    return int(_lib.lib().rldm_train_conv_splits(C.byref(d), 0))


# ---- 1. ops repeat exactly -------------------------------------------------------------------------------------------------------
CONVS = [
    # (Cin, N, taps, stride, mode, split in the default mode)
    (32, 32, 9, 1, 0, True),
    (64, 64, 1, 1, 0, False),           # (one stage: conv_lds_plan cannot split it, see the module docstring)
    (512, 64, 1, 1, 0, True),
    (32, 32, 9, 2, 0, True),
    (32, 32, 9, 1, 1, True),
    (32, 32, 9, 1, 2, True),
]


@pytest.mark.parametrize("Cin,N,taps,stride,mode,split", CONVS)
def test_conv_repeats(Cin, N, taps, stride, mode, split):
    T = _T()
    x = randn((2, 32, 8, Cin), 1)
    k = 3 if taps == 9 else 1
    wf, _ = T.pack_weights(randn((N, Cin, k, k), 2) * 0.1, taps, want_transposed=False)
    bias, row = randn((N,), 3), randn((2, N), 4)
    with det(False):
        assert (splits(x, N, taps, stride, mode) > 1) == split
    with det():
        assert splits(x, N, taps, stride, mode) == 1
    repeats_exactly(lambda: T.conv(x, wf, N, taps, stride, mode, bias=bias, rowadd=row), f"conv {(Cin, N, taps, stride, mode)}")


def _fused_ops(B, W, H, Cin, N, taps, seed):
    T = _T()
    k = 3 if taps == 9 else 1
    x = randn((B, W, H, Cin), seed)
    gn = T.GN(1 + 0.1 * randn((Cin,), seed + 1), 0.1 * randn((Cin,), seed + 2), True, 32, 1e-5)
    wf, wt = T.pack_weights(randn((N, Cin, k, k), seed + 3) * 0.05, taps)
    return x, gn, wf, wt


@pytest.mark.parametrize("W,H,Cin,N,taps", [(64, 16, 64, 64, 9), (256, 16, 64, 64, 9), (64, 16, 64, 64, 1), (64, 16, 96, 64, 9)])
def test_conv_fused_repeats(W, H, Cin, N, taps):
    """want_stats (forward) and the gsrcs / gs_out side (data gradient) of the fused conv.  64 x 16 at B = 2: 32 workgroups, split K with
    a last-arriver epilogue in the default mode; 256 x 16: 64 tiles per image folded in tile order."""
    T = _T()
    B = 2
    x, gn, wf, wt = _fused_ops(B, W, H, Cin, N, taps, 10)
    with det(False):
        if (W, taps) == (64, 9):
            assert splits(x, N, taps) > 1
    with det():
        src = T.Src(x, T.chan_stats(x))
    bias, row, res = randn((N,), 20), randn((B, N), 21), randn((B, W, H, N), 22)
    assert T.conv_fused_ok([src], N, taps, gn=gn, want_stats=True, rowadd=row)
    repeats_exactly(lambda: T.conv_fused([src], wf, N, taps, gn=gn, bias=bias, rowadd=row, res=res, want_stats=True),
                    f"conv_fused want_stats {(W, H, Cin, N, taps)}")
    # data gradient of a conv whose input was act(GN(x)): dy (B, W, H, N) -> dz (B, W, H, Cin), gs
    dy = randn((B, W, H, N), 23)
    assert T.conv_fused_ok([T.Src(dy)], Cin, taps, gsrcs=[src], ggn=gn)
    repeats_exactly(lambda: T.conv_fused([T.Src(dy)], wt, Cin, taps, gsrcs=[src], ggn=gn), f"conv_fused gs_out {(W, H, Cin, N, taps)}")


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("Cin,N,taps", [(32, 32, 9), (64, 64, 1), (64, 64, 9)])
def test_wgrad_bias_repeats(Cin, N, taps, grouped):
    T = _T()
    x, dy = randn((2, 32, 8, Cin), 30), randn((2, 32, 8, N), 31)
    k = 3 if taps == 9 else 1
    pre = randn((N, Cin, k, k), 32)

    def run():
        dw, rows, tot = pre.clone(), torch.empty(2, N, device="cuda"), randn((N,), 33)
        T.wgrad_group(grouped)
        try:
            T.wgrad_bias(dy, x, dw, taps, rows=rows, total=tot)
            if grouped and Cin == 64:
                assert T.wgrad_group_pending() == 1              # (the all-taps kernel's shapes are queued)
            T.wgrad_group_flush()
        finally:
            T.wgrad_group(False)
        return dw, rows, tot

    repeats_exactly(run, f"wgrad_bias {(Cin, N, taps, grouped)}")


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("taps", [9, 1])
def test_wgrad_fused_repeats(taps, grouped):
    T = _T()
    B, W, H, Cin, N = 2, 64, 16, 64, 64
    x, gn, _, _ = _fused_ops(B, W, H, Cin, N, taps, 40)
    with det():
        src = T.Src(x, T.chan_stats(x))
    dy = randn((B, W, H, N), 41)
    assert T.wgrad_fused_ok([src], N, taps, gn=gn)
    k = 3 if taps == 9 else 1

    def run():
        dw, rows, tot = torch.zeros(N, Cin, k, k, device="cuda"), torch.empty(B, N, device="cuda"), torch.zeros(N, device="cuda")
        T.wgrad_group(grouped)
        try:
            T.wgrad_fused(dy, [src], dw, taps, gn=gn, rows=rows, total=tot)
            T.wgrad_group_flush()
        finally:
            T.wgrad_group(False)
        return dw, rows, tot

    repeats_exactly(run, f"wgrad_fused {(taps, grouped)}")


# (2, 32, 8, 64): 2^14 values per image, the one-block-per-(image, group) kernels; (2, 256, 16, 64): 2^18, the slab kernels' threshold
NORM_SHAPES = [(2, 32, 8, 64), (2, 256, 16, 64)]


@pytest.mark.parametrize("shape", NORM_SHAPES)
def test_norm_ops_repeat(shape):
    T = _T()
    B, W, H, Cc = shape
    slab = 1024 % Cc == 0 and W * H * Cc >= (1 << 18)                # (rldm_train_gn_forward / _gn_backward's dispatch)
    assert slab == (shape == NORM_SHAPES[1]) and (W * H >= 4096) == slab    # (and rldm_train_chan_stats's slab size)
    x, dy = randn(shape, 50), randn(shape, 51)
    gamma, beta = 1 + 0.1 * randn((Cc,), 52), 0.1 * randn((Cc,), 53)
    repeats_exactly(lambda: T.chan_stats(x), f"chan_stats {shape}")

    def colsum():
        rows, tot = torch.empty(B, Cc, device="cuda"), torch.ones(Cc, device="cuda")
        T.colsum(dy, rows=rows, total=tot)
        return rows, tot

    repeats_exactly(colsum, f"colsum {shape}")
    repeats_exactly(lambda: T.gn_forward(x, gamma, beta, 32, 1e-5, True), f"gn_forward {shape}")
    with det():
        _, stats = T.gn_forward(x, gamma, beta, 32, 1e-5, True)
        cs = T.chan_stats(x)

    def gn_bwd():
        dg, db = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
        dx = T.gn_backward(x, dy, stats, gamma, beta, 32, True, dg, db)
        return dx, dg, db

    repeats_exactly(gn_bwd, f"gn_backward {shape}")
    gs = randn((B, Cc, 2), 54)
    gn = T.GN(gamma, beta, True, 32, 1e-5)

    def gn_apply():
        dg, db = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
        (dx,) = T.gn_backward_apply(dy, [T.Src(x, cs)], gs, gn, dg, db)
        return dx, dg, db

    repeats_exactly(gn_apply, f"gn_backward_apply {shape}")


def test_mse_and_sqnorm_repeat():
    T = _T()
    pred, target, w = randn((2, 32, 8, 4), 60), randn((2, 4, 32, 8), 61), torch.rand(2).cuda()
    repeats_exactly(lambda: T.mse(pred, target, w), "mse")
    g = randn(((1 << 20) + 3,), 62)
    repeats_exactly(lambda: T.sqnorm(g), "sqnorm")


# ---- 2. nothing lost or counted twice: integer-valued operands ------------------------------------------------------------------
@pytest.mark.parametrize("Cin,N,taps,stride,mode", [c[:5] for c in CONVS])
def test_conv_and_wgrad_exact_on_integers(Cin, N, taps, stride, mode):
    import torch.nn.functional as F
    T = _T()
    B, W, H = 2, 32, 8
    k = 3 if taps == 9 else 1
    x = int_grid((B, Cin, W, H), 201)
    w = int_grid((N, Cin, k, k), 202, -4, 4, exp=-5)
    bias, row = int_grid((N,), 203, -64, 64, exp=-5), int_grid((B, N), 204, -64, 64, exp=-5)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    if mode == 2:
        up = torch.zeros(B, Cin, 2 * W, 2 * H, dtype=torch.float64)
        up[:, :, ::2, ::2] = x64
        xin = up
    else:
        xin = F.interpolate(x64, scale_factor=2.0, mode="nearest") if mode == 1 else x64
    ref = o_ops.circ_conv2d(xin, w64, bias.double(), stride, 1 if taps == 9 else 0) + row.double()[:, :, None, None]
    dy = int_grid(ref.shape, 205)
    ref.backward(dy.double())
    P = B * ref.shape[2] * ref.shape[3]
    assert_exact_bound(U, (Cin * taps * 4, amax(x) * amax(w)), (3, amax(bias, row)))
    assert_exact_bound(1.0, (2 * P, amax(dy) * amax(x)))
    wf, _ = T.pack_weights(w.cuda(), taps, want_transposed=False)
    what = f"{(Cin, N, taps, stride, mode)}"
    with det():
        y = T.conv(nhwc(x), wf, N, taps, stride, mode, bias=bias.cuda(), rowadd=row.cuda())
        assert_bitexact(nchw(y), ref.detach().float(), what="conv " + what)
        if mode == 2:
            return
        for grouped in (False, True):
            dw, rows, tot = torch.zeros_like(w).cuda(), torch.full((B, N), 7.0).cuda(), torch.zeros(N).cuda()
            T.wgrad_group(grouped)
            try:
                T.wgrad_bias(nhwc(dy), nhwc(x), dw, taps, stride, mode, rows=rows, total=tot)
            finally:
                T.wgrad_group(False)
            assert_bitexact(dw.cpu(), w64.grad.float(), names=("n", "cin", "i", "j"), what=f"wgrad_bias {what} grouped={grouped}")
            assert_bitexact(rows.cpu(), dy.sum((2, 3)), names=("image", "n"), what="rows " + what)
            assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what="total " + what)


@pytest.mark.parametrize("shape", NORM_SHAPES)
def test_sums_exact_on_integers(shape):
    T = _T()
    B, W, H, Cc = shape
    x = int_grid((B, Cc, W, H), 301)
    assert_exact_bound(1.0, (B * W * H, amax(x) ** 2))
    with det():
        cs = T.chan_stats(nhwc(x)).cpu()
        rows, tot = torch.full((B, Cc), 5.0).cuda(), torch.full((Cc,), 3.0).cuda()
        T.colsum(nhwc(x), rows=rows, total=tot, rows_accumulate=True)
        sq = T.sqnorm(nhwc(x))
    assert_bitexact(cs[..., 0], x.sum((2, 3)), names=("image", "c"), what="chan_stats sum")
    assert_bitexact(cs[..., 1], (x * x).sum((2, 3)), names=("image", "c"), what="chan_stats sumsq")
    assert_bitexact(rows.cpu(), x.sum((2, 3)) + 5, names=("image", "c"), what="colsum rows")
    assert_bitexact(tot.cpu(), x.sum((0, 2, 3)) + 3, names=("c",), what="colsum total")
    assert float(sq) == float((x.double() ** 2).sum())


def test_mse_exact_on_integers():
    T = _T()
    pred, target = int_grid((2, 4, 32, 8), 310), int_grid((2, 4, 32, 8), 311)       # (2048 elements: the division is by 2^11)
    with det():
        loss, dpred = T.mse(nhwc(pred), target.cuda())
    d = pred.double() - target.double()
    assert float(loss) == float((d * d).sum() / d.numel())
    assert_bitexact(nchw(dpred), (2 * d / d.numel()).float(), what="mse gradient")


@pytest.mark.parametrize("B,C0,C1,N,W,H,taps", [(2, 64, 0, 64, 64, 16, 9), (2, 64, 64, 128, 64, 16, 1), (8, 64, 0, 128, 256, 16, 9)])
def test_fused_gamma0_exact_on_integers(B, C0, C1, N, W, H, taps):
    """tests/test_train_exact.py::test_train_fused_gamma0_exact's construction (gamma = 0: act(GN(x)) = act(beta) per channel) in the
    deterministic mode: y, the per-channel sums of y and the fused weight gradient with its column sums equal the fp64 reference."""
    T = _T()
    h_grid = [k / 8 for k in range(-2, 17)]
    k = 3 if taps == 9 else 1
    Cin = C0 + C1
    x = int_grid((B, Cin, W, H), 601)
    idx = torch.randint(0, len(h_grid), (Cin,), generator=torch.Generator().manual_seed(602))
    h = torch.tensor(h_grid, dtype=torch.float32)[idx]
    beta = silu_targets(h)
    w = int_grid((N, Cin, k, k), 603, -4, 4, exp=-5)
    bias, row, res = int_grid((N,), 604, -64, 64, exp=-5), int_grid((B, N), 605, -64, 64, exp=-5), int_grid((B, N, W, H), 606)
    dy = int_grid((B, N, W, H), 607)
    assert_exact_bound(2.0 ** -8, (Cin * taps, 2 * amax(w)), (1, amax(bias)), (1, amax(row)), (1, amax(res)))
    assert_exact_bound(2.0 ** -3, (B * W * H, 2 * amax(dy)))
    hm = h.double()[None, :, None, None].expand(B, -1, W, H).contiguous()
    w64 = w.double().requires_grad_()
    ref = o_ops.circ_conv2d(hm, w64, bias.double(), 1, 1 if taps == 9 else 0) + row.double()[:, :, None, None] + res.double()
    ref.backward(dy.double())
    ref = ref.detach()
    assert_exact_bound(2.0 ** -8, (1, float(ref.abs().sum((2, 3)).max())))   # the per-channel sums of y: sum of |addends| < 2^24 units
    xd = nhwc(x)
    with det():
        srcs = [T.Src(xd[..., :C0].contiguous())] + ([T.Src(xd[..., C0:].contiguous())] if C1 else [])
        for s in srcs:
            s.cs = T.chan_stats(s.t)
        gn = T.GN(torch.zeros(Cin).cuda(), beta.cuda(), True, 32, 1e-5)
        wf, _ = T.pack_weights(w.cuda(), taps)
        y, cs = T.conv_fused(srcs, wf, N, taps, gn=gn, bias=bias.cuda(), rowadd=row.cuda(), res=nhwc(res), want_stats=True)
        assert_bitexact(nchw(y), ref.float(), what="conv_fused")
        assert_bitexact(cs[..., 0].cpu(), ref.sum((2, 3)).float(), names=("image", "n"), what="conv_fused channel sums")
        assert T.wgrad_fused_ok(srcs, N, taps, gn=gn)
        dw, rows, tot = torch.zeros_like(w).cuda(), torch.empty(B, N).cuda(), torch.zeros(N).cuda()
        T.wgrad_fused(nhwc(dy), srcs, dw, taps, gn=gn, rows=rows, total=tot)
        assert_bitexact(dw.cpu(), w64.grad.float(), names=("n", "cin", "i", "j"), what="wgrad_fused")
        assert_bitexact(rows.cpu(), dy.sum((2, 3)), names=("image", "n"), what="wgrad_fused rows")
        assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what="wgrad_fused total")


# ---- 3. the stated order is the order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NORM_SHAPES + [(3, 11, 7, 36)])      # (77 pixels: a short last partial; 36 channels: a partial tile)
def test_sums_equal_their_host_restatements(shape):
    T = _T()
    x = randn(shape, 70) * 3 + 0.5
    pre_rows, pre_tot = randn((shape[0], shape[3]), 71), randn((shape[3],), 72)
    with det():
        cs = T.chan_stats(x)
        rows, tot = pre_rows.clone(), pre_tot.clone()
        T.colsum(x, rows=rows, total=tot, rows_accumulate=True)
        rows2 = torch.empty_like(rows)
        T.colsum(x, rows=rows2)
        sq = T.sqnorm(x)
    xh = x.cpu().numpy()
    assert np.array_equal(bits(cs).numpy(), T.chan_stats_host(xh).view(np.int32)), "chan_stats"
    r, t = T.colsum_host(xh, rows=pre_rows.cpu().numpy(), total=pre_tot.cpu().numpy())
    assert np.array_equal(bits(rows).numpy(), r.view(np.int32)) and np.array_equal(bits(tot).numpy(), t.view(np.int32)), "colsum"
    assert np.array_equal(bits(rows2).numpy(), T.colsum_host(xh)[0].view(np.int32)), "colsum rows, written"
    assert float(sq) == float(T.sqnorm_host(xh)), "sqnorm"


def test_mse_and_sqnorm_equal_their_host_restatements():
    T = _T()
    pred, target, w = randn((2, 32, 8, 4), 80), randn((2, 4, 32, 8), 81), torch.rand(2).cuda()
    g = randn(((1 << 20) + 3,), 82)                                   # (4097 blocks -> capped at 2048: three values per thread)
    with det():
        loss, _ = T.mse(pred, target, w)
        loss1, _ = T.mse(pred, target)
        sq = T.sqnorm(g)
    assert float(loss) == float(T.mse_host(pred.cpu().numpy(), target.cpu().numpy(), w.cpu().numpy()))
    assert float(loss1) == float(T.mse_host(pred.cpu().numpy(), target.cpu().numpy()))
    assert float(sq) == float(T.sqnorm_host(g.cpu().numpy()))


@pytest.mark.parametrize("B,W,H,Cin,N,taps", [(2, 64, 16, 64, 64, 9), (2, 256, 16, 64, 64, 9), (2, 64, 16, 64, 64, 1), (2, 64, 16, 96, 64, 9),
                                              (8, 256, 16, 64, 128, 9), (2, 64, 4, 128, 192, 1)])
def test_fused_conv_statistics_equal_chan_stats_of_its_output(B, W, H, Cin, N, taps):
    """One canonical order: halo <64> / <128>, lds <64, 128> (1x1), lds <32, 64> (96 channels) epilogues against rldm_train_chan_stats
    on the stored y, bit for bit, and against the numpy restatement."""
    T = _T()
    x, gn, wf, _ = _fused_ops(B, W, H, Cin, N, taps, 90)
    bias, res = randn((N,), 91), randn((B, W, H, N), 92)
    with det():
        src = T.Src(x, T.chan_stats(x))
        y, cs = T.conv_fused([src], wf, N, taps, gn=gn, bias=bias, res=res, want_stats=True)
        cs_y = T.chan_stats(y)
    assert torch.equal(bits(cs), bits(cs_y))
    assert np.array_equal(bits(cs).numpy(), T.chan_stats_host(y.cpu().numpy()).view(np.int32))


# ---- 4. whole step, small -----------------------------------------------------------------------------------------------------------
def _batches(n, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(shape, generator=g).cuda(), torch.randint(0, 1000, (shape[0],), generator=g).cuda(),
             torch.randn(shape, generator=g).cuda(), torch.rand(shape[0], generator=g).cuda()) for _ in range(n)]


def _state_bits(tr):
    return [bits(t) for t in (tr.params, tr.exp_avg, tr.exp_avg_sq, tr.ema)]


@pytest.mark.parametrize("kind", ["eager", "accumulate", "graphed"])
def test_small_steps_repeat(kind):
    from rangeldm_amd import training as TR
    T = _T()
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    kw = dict(lr=1e-3, lr_warmup_steps=2, total_steps=40, use_ema=True, deterministic=True,
              gradient_accumulation_steps=2 if kind == "accumulate" else 1)
    n = 4 if kind == "accumulate" else 3
    batches = _batches(n, (2, 4, 32, 8), 5)
    states, losses = [], []
    for _ in range(2):
        tr = TR.UNetTrainer(cfg, sd, **kw)
        assert tr.deterministic
        step = tr.train_step_graphed if kind == "graphed" else tr.train_step
        ls = [bits(step(x, t, target, w, pos_encoding=True)) for x, t, target, w in batches]
        assert not T.deterministic_enabled()
        torch.cuda.synchronize()
        states.append(_state_bits(tr))
        losses.append(ls)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), *states):
        assert torch.equal(a, b), f"{kind}: {name} differ in {int((a != b).sum())} of {a.numel()} elements"
    assert all(torch.equal(a, b) for a, b in zip(*losses)), f"{kind}: losses differ"
    assert float(states[0][1].abs().max()) > 0                        # (the optimizer ran)


# ---- 5. whole step, fused tape -------------------------------------------------------------------------------------------------------
_default_grads = {}


def _two_passes(cfg, sd, x, t, target, deterministic, fused):
    from rangeldm_amd import training as TR
    T = _T()
    tr = TR.UNetTrainer(cfg, sd, use_ema=False, deterministic=deterministic)
    tr.fused_tape = fused
    assert tr.fused_shape_ok(*[x.shape[i] for i in (0, 2, 3)]) == fused
    out = []
    for _ in range(2):
        pred = tr.forward(x, t, pos_encoding=True)
        assert tr.last_forward_fused == fused
        with det(deterministic):
            loss, dpred = T.mse(pred, target)
        tr.backward(dpred)
        out.append((bits(loss), tr.grads.clone()))
        tr.grads.zero_()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_fused_shape_gradients_repeat_and_stay_inside_the_default_gate(fused):
    cfg = UNetConfig(sample_size=(256, 16), block_out_channels=(64, 64, 128, 128))
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="trd.")
    g = torch.Generator().manual_seed(21)
    x, target = torch.randn(2, 4, 256, 16, generator=g).cuda(), torch.randn(2, 4, 256, 16, generator=g).cuda()
    t = torch.tensor([101, 902]).cuda()
    (la, ga), (lb, gb) = _two_passes(cfg, sd, x, t, target, True, fused)
    assert torch.equal(la, lb) and torch.equal(bits(ga), bits(gb)), int((bits(ga) != bits(gb)).sum())
    (_, gd), _ = _two_passes(cfg, sd, x, t, target, False, fused)
    r = rel(ga, gd)
    print(f"deterministic against default gradients (fused_tape={fused}): rel {r:.3e}")
    assert r < 5e-3, r                                               # (the run-to-run gate of tests/test_training.py)


def test_full_width_gradients_repeat():
    """The RangeLDM width (128, 128, 256, 256), B = 2: forward + backward twice, bit for bit."""
    cfg = UNetConfig()
    sd = synth_state_dict(unet_param_shapes(cfg))
    g = torch.Generator().manual_seed(22)
    x, target = torch.randn(2, 4, 256, 16, generator=g).cuda(), torch.randn(2, 4, 256, 16, generator=g).cuda()
    t = torch.tensor([77, 640]).cuda()
    (la, ga), (lb, gb) = _two_passes(cfg, sd, x, t, target, True, True)
    assert torch.equal(la, lb) and torch.equal(bits(ga), bits(gb)), int((bits(ga) != bits(gb)).sum())


# ---- 6. the switch is scoped -----------------------------------------------------------------------------------------------------------
def test_switch_is_scoped_to_the_trainer_calls():
    from rangeldm_amd import training as TR
    T = _T()
    cfg = UNetConfig(**SMALL)
    sd = synth_state_dict(unet_param_shapes(cfg), prefix="tr.")
    (x, t, target, w), = _batches(1, (2, 4, 32, 8), 9)
    probe = torch.empty(2, 32, 8, 32, device="cuda")
    assert not T.deterministic_enabled()
    before = splits(probe, 32, 9)
    assert before > 1

    def default_grads():
        tr = TR.UNetTrainer(cfg, sd, use_ema=False)
        assert not tr.deterministic
        tr.backward(T.mse(tr.forward(x, t, pos_encoding=True), target)[1])
        return tr.grads.clone()

    g0 = default_grads()
    tr = TR.UNetTrainer(cfg, sd, use_ema=False, deterministic=True)
    for prev in (False, True):                                      # (the PREVIOUS value comes back, whichever it was)
        with det(prev):
            pred = tr.forward(x, t, pos_encoding=True)
            assert T.deterministic_enabled() == prev
            tr.backward(T.mse(pred, target)[1])
            assert T.deterministic_enabled() == prev
            tr.optimizer_step()
            assert T.deterministic_enabled() == prev
            tr.train_step(x, t, target, w, pos_encoding=True)
            assert T.deterministic_enabled() == prev
            with pytest.raises(ValueError):
                tr.forward(x[:, :2], t, pos_encoding=True)           # (3 channels with the marker: the UNet expects 5)
            assert T.deterministic_enabled() == prev
            with pytest.raises(ValueError):
                tr.train_step(x[:, :2], t, target, w, pos_encoding=True)
            assert T.deterministic_enabled() == prev
    T.set_zero_arena(None)                                          # (the failed forwards left theirs installed)
    assert not T.deterministic_enabled()
    assert splits(probe, 32, 9) == before
    with det():
        assert splits(probe, 32, 9) == 1
    assert rel(default_grads(), g0) < 5e-3
