"""GPU, bit-exact: the training conv / weight-gradient kernels (rangeldm_amd/csrc/train_conv.hip, train_wgrad.hip) on integer-grid operands.

Activations and gradients are integers in [-3, 3], weights {-4 .. 4} * 2^-5, bias / row / residual on the 2^-5 grid: every product and
every sum is exact in fp32 in any order (asserted per case), so the fp32 outputs -- conv, data gradient, weight gradient, column sums
-- must EQUAL the fp64 reference, split-K atomics and partial-tile reductions included (which also makes these tests deterministic).
Routing depends on the shape only; the cases below are chosen to reach every branch of train_conv_impl / conv_lds_plan /
train_wgrad_impl, named per case.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as o_ops
from tests.hip_util import amax, assert_bitexact, assert_exact_bound, int_grid, silu_targets

pytestmark = pytest.mark.gpu
U = 2.0 ** -5


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def _exact(y_nhwc, ref, what):
    assert_bitexact(nchw(y_nhwc), ref.float(), what=what)


CASES = [
    # (B, Cin, N, W, H, taps, stride, mode)   conv forward route / weight-gradient route
    (3, 48, 32, 8, 4, 9, 1, 0),         # tr_conv_kernel<true> (Cin % 32 != 0, Cin % 16 == 0) / tr_wgrad_kernel + reduce
    (2, 5, 32, 16, 8, 9, 1, 0),         # tr_conv_kernel<false> (Cin % 16 != 0) / tr_wgrad_kernel
    (5, 128, 512, 1, 1, 1, 1, 0),       # direct kernel on 5 rows (P < 64): a Linear
    (2, 32, 64, 16, 8, 9, 1, 0),        # lds <32, 64> split K / tr_wgrad_kernel (Cin % 64 != 0)
    (2, 96, 40, 8, 4, 1, 1, 0),         # lds <32, 128> (1x1: wide tile), one split
    (2, 64, 64, 16, 8, 9, 1, 0),        # lds <64, 64> split K / tr_wgrad2_kernel<9> (partial tiles + reduce)
    (2, 512, 128, 16, 4, 1, 1, 0),      # lds <64, 128> split K (1x1) / tr_wgrad2_kernel<1> (adds into dw)
    (16, 128, 128, 128, 8, 1, 1, 0),    # lds <64, 128> one split (1x1, 256 workgroups) / tr_wgrad2_kernel<1>
    (2, 64, 64, 16, 8, 9, 2, 0),        # stride 2 (lds split) / data gradient by zero insertion (mode 2) / tr_wgrad_kernel
    (2, 64, 64, 8, 4, 9, 1, 1),         # nearest x2 folded (mode 1) / data gradient at 2x + sum2x2 / tr_wgrad2_kernel<9> mode 1
    (4, 64, 128, 256, 16, 9, 1, 0),     # tr_conv_halo_kernel<64> (H = 16) / wgrad2<9>
    (8, 64, 128, 256, 16, 9, 1, 0),     # tr_conv_halo_kernel<128>
    (16, 64, 256, 64, 4, 9, 1, 0),      # halo<64> on 4 beams
    (32, 64, 256, 64, 2, 9, 1, 0),      # halo<64> on 2 beams (three halo passes)
    (3, 64, 128, 32, 4, 9, 1, 0),       # lds <64, 64> split / wgrad2<9>, H = 4
    (9, 64, 64, 64, 16, 9, 1, 0),       # odd batch, H = 16
]


def _ops(case):
    B, Cin, N, W, H, taps, stride, mode = case
    k = 3 if taps == 9 else 1
    x = int_grid((B, Cin, W, H), 201)
    w = int_grid((N, Cin, k, k), 202, -4, 4, exp=-5)
    bias, row = int_grid((N,), 203, -64, 64, exp=-5), int_grid((B, N), 204, -64, 64, exp=-5)
    return x, w, bias, row


def _fwd64(x, w, bias, stride, mode, taps):
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if mode == 1 else x
    return o_ops.circ_conv2d(xin, w, bias, stride, 1 if taps == 9 else 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_train_conv_dgrad_wgrad_exact(case):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, taps, stride, mode = case
    x, w, bias, row = _ops(case)
    xd64, wd64 = x.double().requires_grad_(), w.double().requires_grad_()
    ref = _fwd64(xd64, wd64, bias.double(), stride, mode, taps) + row.double()[:, :, None, None]
    Wo, Ho = ref.shape[2], ref.shape[3]
    P = B * Wo * Ho
    dy = int_grid(ref.shape, 205)
    ref.backward(dy.double())
    ref = ref.detach()
    assert_exact_bound(U, (Cin * taps * 4, amax(x) * amax(w)), (3, amax(bias, row)), (2, amax(dy)))
    assert_exact_bound(U, (N * taps * 4, amax(dy) * amax(w)))                             # data gradient (x 4: sum2x2)
    assert_exact_bound(1.0, (2 * P, amax(dy) * amax(x)))                                  # dw (twice), rows, total
    wf, wt = T.pack_weights(w.cuda(), taps)
    xd = nhwc(x)
    what = f"{case}"
    y = T.conv(xd, wf, N, taps, stride, mode, bias=bias.cuda(), rowadd=row.cuda())
    torch.cuda.synchronize()
    _exact(y, ref, "conv " + what)
    # residual + accumulate: y2 = y + conv + res
    y2 = T.conv(xd, wf, N, taps, stride, mode, res=y, out=y.clone(), accumulate=True)
    _exact(y2, 3 * ref - bias.double()[None, :, None, None] - row.double()[:, :, None, None], "conv res + accumulate " + what)
    # rowadd of a column slice whose row stride is not a multiple of 4: the direct kernel at the same shape
    wide = torch.zeros(B, N + 1)
    wide[:, :N] = row
    wide = wide.cuda()
    y3 = T.conv(xd, wf, N, taps, stride, mode, bias=bias.cuda(), rowadd=wide[:, :N])
    _exact(y3, ref, "conv (direct kernel: unaligned rowadd) " + what)
    # data gradient
    dyd = nhwc(dy)
    if stride == 2:
        dx = T.conv(dyd, wt, Cin, taps, 1, 2)
    elif mode == 1:
        dx = T.sum2x2(T.conv(dyd, wt, Cin, taps, 1, 0))
    else:
        dx = T.conv(dyd, wt, Cin, taps, 1, 0)
    _exact(dx, xd64.grad, "data gradient " + what)
    # weight gradient, twice into one buffer
    dw = torch.zeros_like(w).cuda()
    T.wgrad(dyd, xd, dw, taps, stride, mode)
    torch.cuda.synchronize()
    assert_bitexact(dw.cpu(), wd64.grad.float(), names=("n", "cin", "i", "j"), what="wgrad " + what)
    T.wgrad(dyd, xd, dw, taps, stride, mode)
    assert_bitexact(dw.cpu(), 2 * wd64.grad.float(), names=("n", "cin", "i", "j"), what="wgrad twice " + what)
    # with the bias / row sums from the same pass; rows as a column slice, the columns around untouched
    dw3, rows3, tot3 = torch.zeros_like(dw), torch.full((B, N + 4), 7.0).cuda(), torch.zeros(N).cuda()
    T.wgrad_bias(dyd, xd, dw3, taps, stride, mode, rows=rows3[:, 4:], total=tot3)
    torch.cuda.synchronize()
    assert_bitexact(dw3.cpu(), wd64.grad.float(), names=("n", "cin", "i", "j"), what="wgrad_bias " + what)
    assert_bitexact(rows3[:, 4:].cpu(), dy.sum((2, 3)), names=("image", "n"), what="wgrad_bias rows " + what)
    assert_bitexact(tot3.cpu(), dy.sum((0, 2, 3)), names=("n",), what="wgrad_bias total " + what)
    assert float((rows3[:, :4] - 7.0).abs().max()) == 0
    rows, tot = torch.full((B, N), 1.0).cuda(), torch.zeros(N).cuda()
    T.colsum(dyd, rows=rows, total=tot, rows_accumulate=True)
    assert_bitexact(rows.cpu(), dy.sum((2, 3)) + 1, names=("image", "n"), what="colsum rows " + what)
    assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what="colsum total " + what)


# ---- grouped weight gradients: every class, several layers in one flush, dw pre-filled -----------------------------------------------
GROUP_LAYERS = [
    # (B, Cin, N, W, H, taps, mode)                       class
    (2, 64, 64, 32, 16, 9, 0),          # 3x3 V3 (H = 16)
    (4, 128, 64, 24, 8, 9, 0),          # 3x3 V3 (H = 8, W = 24: chunk-bounded dy segments)
    (2, 64, 128, 32, 4, 9, 0),          # 3x3 round-5 staging (H = 4)
    (8, 64, 64, 32, 2, 9, 0),           # 3x3 round-5 staging (H = 2, few chunks)
    (2, 64, 64, 8, 4, 9, 1),            # 3x3, nearest x2 (mode 1: never V3)
    (2, 128, 64, 16, 8, 1, 0),          # 1x1 V3
    (4, 128, 128, 32, 4, 1, 0),         # 1x1 round-5 staging
]


def test_train_wgrad_grouped_every_class_exact():
    from rangeldm_amd import train_ops as T
    layers = []
    for i, (B, Cin, N, W, H, taps, mode) in enumerate(GROUP_LAYERS):
        k = 3 if taps == 9 else 1
        x = int_grid((B, Cin, W, H), 300 + i)
        Wo, Ho = (W, H) if mode == 0 else (2 * W, 2 * H)
        dy = int_grid((B, N, Wo, Ho), 320 + i)
        xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if mode == 1 else x.double()
        w64 = torch.zeros(N, Cin, k, k, dtype=torch.float64, requires_grad=True)
        o_ops.circ_conv2d(xin, w64, None, 1, 1 if taps == 9 else 0).backward(dy.double())
        pre = int_grid((N, Cin, k, k), 340 + i, -100, 100)
        assert_exact_bound(1.0, (B * Wo * Ho * (4 if mode == 1 else 1), 9.0), (1, amax(pre)))
        layers.append((x, dy, taps, mode, pre, w64.grad, (B, Cin, N, W, H, taps, mode)))
    dws, rowss, tots, keep = [], [], [], []
    T.wgrad_group(True)
    try:
        for x, dy, taps, mode, pre, _, _ in layers:
            dw, rows, tot = pre.clone().cuda(), torch.zeros(x.shape[0], dy.shape[1]).cuda(), torch.zeros(dy.shape[1]).cuda()
            keep.append((nhwc(dy), nhwc(x)))                # (queued operands stay alive until the flush)
            T.wgrad_bias(*keep[-1], dw, taps, 1, mode, rows=rows, total=tot)
            dws.append(dw), rowss.append(rows), tots.append(tot)
        assert T.wgrad_group_pending() == len(layers)
        T.wgrad_group_flush()
        assert T.wgrad_group_pending() == 0
    finally:
        T.wgrad_group(False)
    torch.cuda.synchronize()
    for (x, dy, taps, mode, pre, g, case), dw, rows, tot in zip(layers, dws, rowss, tots):
        assert_bitexact(dw.cpu(), pre + g.float(), names=("n", "cin", "i", "j"), what=f"grouped wgrad {case}")
        assert_bitexact(rows.cpu(), dy.sum((2, 3)), names=("image", "n"), what=f"grouped rows {case}")
        assert_bitexact(tot.cpu(), dy.sum((0, 2, 3)), names=("n",), what=f"grouped total {case}")


# ---- the deferred reduction ---------------------------------------------------------------------------------------------------------
WG = (2, 64, 64, 16, 8)             # tr_wgrad2_kernel<9>: partial tiles, whose reduction is deferred
RIDERS = {
    "split-k": (2, 64, 64, 16, 8, 1),        # lds <64, 64>, split K: the reduction's planes follow the split planes
    "halo": (4, 64, 128, 256, 16, 1),        # tr_conv_halo_kernel<64>
    "lds-one-split": (16, 128, 128, 128, 8, 0),   # 1x1 lds <64, 128>, one split
    "direct": (3, 48, 32, 8, 4, 1),          # tr_conv_kernel: flushes first
    "other-stream": (2, 64, 64, 16, 8, 1),   # a conv on another stream: flushes on the weight gradient's stream
    "flush": None,                           # rldm_train_flush_reduce
}


@pytest.mark.parametrize("rider", list(RIDERS))
def test_train_deferred_reduction_exact(rider):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H = WG
    x, dy = int_grid((B, Cin, W, H), 401), int_grid((B, N, W, H), 402)
    w64 = torch.zeros(N, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    o_ops.circ_conv2d(x.double(), w64, None).backward(dy.double())
    pre = int_grid((N, Cin, 3, 3), 403, -100, 100)
    assert_exact_bound(1.0, (B * W * H, 9.0), (1, amax(pre)))
    dw = pre.clone().cuda()
    y = ref = None
    T.defer_reduce(True)
    try:
        T.wgrad(nhwc(dy), nhwc(x), dw, 9)
        assert T.reduce_pending()
        if RIDERS[rider] is None:
            T.flush_reduce()
        else:
            cb, cc, cn, cw, chh, k = RIDERS[rider]
            cx, cwt, cbias = int_grid((cb, cc, cw, chh), 404), int_grid((cn, cc, 2 * k + 1, 2 * k + 1), 405, -4, 4, exp=-5), \
                int_grid((cn,), 406, -64, 64, exp=-5)
            assert_exact_bound(U, (cc * (2 * k + 1) ** 2, amax(cx) * amax(cwt)), (1, amax(cbias)))
            wf, _ = T.pack_weights(cwt.cuda(), 9 if k else 1, want_transposed=False)
            ref = o_ops.circ_conv2d(cx.double(), cwt.double(), cbias.double(), 1, k)
            xdev, bdev = nhwc(cx), cbias.cuda()
            if rider == "other-stream":
                s2 = torch.cuda.Stream()
                s2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s2):
                    y = T.conv(xdev, wf, cn, 9 if k else 1, bias=bdev)
                torch.cuda.current_stream().wait_stream(s2)
            else:
                y = T.conv(xdev, wf, cn, 9 if k else 1, bias=bdev)
        assert not T.reduce_pending(), "the reduction is still pending"
    finally:
        T.defer_reduce(False)
    torch.cuda.synchronize()
    assert_bitexact(dw.cpu(), pre + w64.grad.float(), names=("n", "cin", "i", "j"), what=f"deferred reduction ({rider})")
    if y is not None:
        _exact(y, ref, f"conv carrying the reduction ({rider})")


# ---- rows-wise Linear kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,N", [(8, 512, 4352), (3, 40, 24), (16, 4352, 512)])
def test_linear_rows_exact(B, K, N):
    from rangeldm_amd import train_ops as T
    x = int_grid((B, K), 501)
    w = int_grid((N, K), 502, -4, 4, exp=-5)
    bias = int_grid((N,), 503, -64, 64, exp=-5)
    dy = int_grid((B, N), 504)
    assert_exact_bound(U, (K, amax(x) * amax(w)), (1, amax(bias)))
    assert_exact_bound(U, (N, amax(dy) * amax(w)))
    assert_exact_bound(1.0, (2 * B, amax(dy) * amax(x)))
    wf, wt = T.pack_weights(w.cuda(), 1)
    wide = torch.zeros(B, K + 8).cuda()
    wide[:, 4:4 + K] = x.cuda()
    y = T.linear_rows(wide[:, 4:4 + K], wf, N, bias=bias.cuda())
    torch.cuda.synchronize()
    assert_bitexact(y.cpu(), (x.double() @ w.double().T + bias.double()).float(), names=("row", "n"), what="linear_rows")
    assert_bitexact(T.linear_rows(dy.cuda(), wt, K).cpu(), (dy.double() @ w.double()).float(), names=("row", "k"), what="linear_rows dgrad")
    dw, db = torch.zeros(N, K).cuda(), torch.zeros(N).cuda()
    for _ in range(2):
        T.linear_rows_wgrad(dy.cuda(), wide[:, 4:4 + K], dw, db)
    torch.cuda.synchronize()
    assert_bitexact(dw.cpu(), (2 * dy.double().T @ x.double()).float(), names=("n", "k"), what="linear_rows_wgrad")
    assert_bitexact(db.cpu(), 2 * dy.sum(0), names=("n",), what="linear_rows_wgrad bias")


# ---- fused forms with gamma = 0: act(GN(x)) is act(beta) per channel ------------------------------------------------------------------
H_GRID = [k / 8 for k in range(-2, 17)]


@pytest.mark.parametrize("B,C0,C1,N,W,H,taps", [
    (8, 256, 0, 256, 32, 2, 9),          # split-K launch, the tile's last arriver runs the statistics epilogue
    (8, 256, 128, 256, 64, 4, 9),        # two sources, split K
    (4, 128, 0, 128, 256, 16, 9),        # halo <64, fused>
    (8, 128, 0, 128, 256, 16, 9),        # halo <128, fused>
    (2, 128, 128, 384, 128, 8, 1),       # 1x1, two sources
    (2, 96, 0, 64, 32, 4, 9),            # 32-channel chunks
    (3, 64, 64, 64, 64, 2, 9),           # three halo passes, two sources
])
def test_train_fused_gamma0_exact(B, C0, C1, N, W, H, taps):
    from rangeldm_amd import train_ops as T
    k = 3 if taps == 9 else 1
    Cin = C0 + C1
    x = int_grid((B, Cin, W, H), 601)
    idx = torch.randint(0, len(H_GRID), (Cin,), generator=torch.Generator().manual_seed(602))
    h = torch.tensor(H_GRID, dtype=torch.float32)[idx]
    beta = silu_targets(h)
    w = int_grid((N, Cin, k, k), 603, -4, 4, exp=-5)
    bias, row, res = int_grid((N,), 604, -64, 64, exp=-5), int_grid((B, N), 605, -64, 64, exp=-5), int_grid((B, N, W, H), 606)
    dy = int_grid((B, N, W, H), 607)
    assert_exact_bound(2.0 ** -8, (Cin * taps, 2 * amax(w)), (1, amax(bias)), (1, amax(row)), (1, amax(res)))
    assert_exact_bound(2.0 ** -3, (B * W * H, 2 * amax(dy)))
    hm = h.double()[None, :, None, None].expand(B, -1, W, H).contiguous().requires_grad_(False)
    w64 = w.double().requires_grad_()
    ref = o_ops.circ_conv2d(hm, w64, bias.double(), 1, 1 if taps == 9 else 0) + row.double()[:, :, None, None] + res.double()
    ref.backward(dy.double())
    xd = nhwc(x)
    srcs = [T.Src(xd[..., :C0].contiguous())] + ([T.Src(xd[..., C0:].contiguous())] if C1 else [])
    for s in srcs:
        s.cs = T.chan_stats(s.t)
    gn = T.GN(torch.zeros(Cin).cuda(), beta.cuda(), True, 32, 1e-5)
    wf, _ = T.pack_weights(w.cuda(), taps)
    what = f"{(B, C0, C1, N, W, H, taps)}"
    y, _ = T.conv_fused(srcs, wf, N, taps, gn=gn, bias=bias.cuda(), rowadd=row.cuda(), res=nhwc(res), want_stats=True)
    _exact(y, ref.detach(), "conv_fused + statistics " + what)
    y1 = T.conv_fused(srcs, wf, N, taps, gn=gn, bias=bias.cuda(), rowadd=row.cuda(), res=nhwc(res))
    _exact(y1, ref.detach(), "conv_fused " + what)
    if T.wgrad_fused_ok(srcs, N, taps, gn=gn):
        dyd = nhwc(dy)
        dw = torch.zeros_like(w).cuda()
        T.wgrad_fused(dyd, srcs, dw, taps, gn=gn)
        torch.cuda.synchronize()
        assert_bitexact(dw.cpu(), w64.grad.float(), names=("n", "cin", "i", "j"), what="wgrad_fused " + what)
        dw2 = torch.zeros_like(dw)
        T.wgrad_group(True)
        try:
            T.wgrad_fused(dyd, srcs, dw2, taps, gn=gn)
            assert T.wgrad_group_pending() == 1
        finally:
            T.wgrad_group(False)
        torch.cuda.synchronize()
        assert_bitexact(dw2.cpu(), w64.grad.float(), names=("n", "cin", "i", "j"), what="grouped wgrad_fused " + what)
