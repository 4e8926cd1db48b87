"""GPU: the training kernels (rangeldm_amd/csrc/train.hip, train_conv.hip, train_wgrad.hip, train_norm.hip, train_attn.hip) on operands placed as the trainers place them.

Every other kernel test allocates each operand as its own torch tensor.  The trainers do not: parameters and gradients are views of flat
buffers packed end to end (FlatParameters._init_parameters), split-K outputs are slices of one pre-zeroed arena (ZeroArena.take), and the
wrappers' own outputs come from a caching allocator that hands back the block just freed.  Here every operand is a view between guards
(tests/hip_util.py: place / assert_placement; tests/test_placement_host.py tests those):

  inputs    between quiet NaNs: a load past an input that is consumed -- also as x * 0 -- turns the result into NaN; an input that was
            written shows bit for bit
  outputs   between finite sentinels, the interior pre-filled with a NaN pattern: a store before or past the view, and an element that
            is never written, show
  accumulating outputs (dw, total, rows, dx / out with accumulate, arena slices) carry integer pre-fill values that enter the reference

Placements.  "r" below is RESIDUES: offset % 4 (floats) of every parameter / gradient view of VAEDecoderTrainer, VAETrainer and
UNetTrainer (full and nuScenes), derived on the CPU by tests.hip_util.trainer_residues (tests/test_placement_host.py asserts the list
here equals it).  It is [0] today: the VAE's 2-float decoder.conv_out.bias is the last parameter of both VAE trainers' buffers, so no
view starts behind it.  Activations, dy, conv outputs, statistics and the packed bf16 weights are at residue 0 (torch allocations and the
arena are 16-byte aligned).

  op                                               placed                                                   residues   modes
  conv / data gradient / wgrad / wgrad_bias /      x, dy, res, rowadd (column slice), wf, wt in; y, dx out;   bias, dw,  both
    colsum, 14 cases; accumulate into `out`        y acc; rows acc (column slice); rows out                   total: r
  two split-K convs from one ZeroArena             the arena itself is the placed buffer                      0          default
  grouped weight gradients (H <= 8 layers)         dy, x in; ONE flat [w0|b0|w1|b1|...] acc, no guards       r          both
                                                   between layers: a dw's neighbour is the next layer's
  deferred reduction (split-k, flush)              dy, x in; dw acc; the rider's y out                        dw: r      both
  conv_fused / wgrad_fused, gamma = 0              sources, cs, res, rowadd in; y, dz out; cs_out, gs_out    gamma,     both
                                                   acc; dw acc                                                beta,
                                                                                                              bias, dw: r
  linear_rows / data gradient / linear_rows_wgrad  x (column slice), dy, wf, wt in; y out / acc               bias, dw,  both
                                                                                                              dbias: r
  add, copy_channels, sum2x2, pack_input,          every operand                                              0          both
    unpack_output
  pack_weights                                     w in (r); wf, wt bf16 out                                  w: r       both
  mse, l1, sqnorm, colsum, chan_stats              every operand; dpred and the fp64 loss words out           0          both
  gn_forward / gn_backward                         x, dy in; y, stats, scratch, dx out; dx acc                gamma,     both
                                                                                                              beta,
                                                                                                              dgamma,
                                                                                                              dbeta: r
  chan_stats, gn_backward_apply                    every operand; cs acc; dsts out / acc                      gamma,     both
                                                                                                              dgamma,
                                                                                                              dbeta: r
  attention_forward / _backward, qkv forms         q, k, v, qkv, o, dO, lse in; o, lse, delta, dq, dk, dv,    0          both
                                                   dqkv out
  silu, silu_backward, timestep_embedding,         every operand but the int64 timesteps; kl (fp64) out       0          both
    gaussian, gaussian_backward

What the read-through of the flat-buffer operands found (one line per operand class; "scalar" = 4-byte accesses only).  FIXED = the
cast to a 16-byte type, which claims an alignment these views do not promise, is replaced by four element accesses (tr_load4 /
tr_store4 in train_common.h: alignment 4; the compiler may still merge them where the target takes a 16-byte access at 4-byte alignment):
  bias     16-byte loads in tr_tile_epilogue, the register epilogue of tr_conv_lds_kernel and tr_conv_halo_kernel: FIXED;
           tr_conv_kernel, the split-K epilogue and tr_linear_rows_kernel: scalar
  gamma,   16-byte loads in tr_gn_fwd_fused_vec_kernel, tr_gn_fwd_vec_kernel and tr_gn_bwd_apply_vec_kernel: FIXED;
  beta     tr_gn_coeffs / tr_gn_coeffs_tile / the weight-gradient staging (fused forms), the scalar and slab GroupNorm kernels,
           tr_gn_bwd_apply2_kernel: scalar
  dw       a 16-byte load + store in tr_linear_rows_wgrad_kernel: FIXED; tr_wgrad_kernel's partial planes,
           tr_wgrad2_body (atomics, the GROUP `*dst +=`, the last arriver's sum), tr_wgrad_reduce_items (16-byte loads of the library's
           own partial planes, scalar `dw[...] +=`) and tr_wgrad_reduce_kernel: scalar
  total,   unsafeAtomicAdd of one float (tr_wgrad2_body, tr_colsum_kernel), tr_colsum_finish_kernel, `dbias[n] +=`: scalar
  dbias
  dgamma,  unsafeAtomicAdd of one float (tr_gn_bwd_reduce_kernel, the slab kernel), tr_fold_rows_kernel, `a.dgamma[c] +=` in
  dbeta    tr_gn_bwd_apply2_kernel: scalar
  weights  (fp32 masters read by the pack kernels) tr_pack_tile_fast's 16-byte loads are already chosen from `param_offset & 3`; the
           element-wise kernels are scalar
  Nothing else in these files looks at a pointer's alignment except rldm_train_l1 (pred / dpred, activations).

Ops on integer grids (tests/test_train_exact.py's operands and bounds) must EQUAL the fp64 reference; the others are compared with the
same call on plain torch allocations -- bit for bit in the deterministic mode and wherever the default route has no floating-point
atomics, else with the tolerance the op's test in tests/test_train_ops.py states (named where used)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as o_ops
from rangeldm_amd import _lib
from tests.hip_util import (GUARD, RefCache, amax, assert_bitexact, assert_exact_bound, assert_placement, int_grid, place, rel_l2,
                            silu_targets, trainer_residues)
from tests.test_train_exact import GROUP_LAYERS, H_GRID, RIDERS, WG, U, nchw
from tests.test_train_ops import TOL_F32, TOL_MM
from tests.test_vae_training_gpu import mode

pytestmark = pytest.mark.gpu
RESIDUES = sorted(set().union(*trainer_residues().values()))
MODES = [False, True]
MODE_IDS = ["default", "deterministic"]
DEV = "cuda"
REFS = RefCache(cap=32)
both_modes = pytest.mark.parametrize("det", MODES, ids=MODE_IDS)
residues = pytest.mark.parametrize("r", RESIDUES, ids=lambda r: f"residue{r}")


def p_in(r=0, **tensors):
    return place(tensors, GUARD + r, "in", device=DEV)


def p_out(r=0, dtype=torch.float32, **shapes):
    return place(shapes, GUARD + r, "out", device=DEV, dtype=dtype)


def p_acc(r=0, **tensors):
    return place(tensors, GUARD + r, "acc", device=DEV)


def done(what, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert_placement(b, f"{what} [{b.kind} buffer {'/'.join(b.names)}]")


def call(fn, *args):
    """the C ABI directly (where a train_ops wrapper would allocate the outputs itself): tensors go in as pointers"""
    a = [C.c_void_p(v.data_ptr()) if torch.is_tensor(v) else v for v in args]
    _lib.check(getattr(_lib.lib(), fn)(*a, _lib.stream_ptr(torch.device(DEV))), fn)


def cl(t):
    """NCHW host tensor -> NHWC host tensor (placed by the caller)"""
    return t.permute(0, 2, 3, 1).contiguous()


def exact(got, want, what, names=None):
    got, want = got.detach().cpu(), want.detach().cpu().to(got.dtype)
    assert_bitexact(got.float(), want.float(), names=names or tuple(f"d{i}" for i in range(got.dim())), what=what)


def same(got, want, what, tol=None):
    """placement independence: bit for bit, or (a route that meets in floating-point atomics) within `tol` relative L2"""
    if tol is None:
        g, w = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
        assert g.shape == w.shape, what
        bad = (g.view(-1) != w.view(-1)) | torch.isnan(g.view(-1))
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {g.numel()} elements differ from the plain-allocation call; first at " \
                                    f"flat index {int(bad.nonzero()[0])}"
    else:
        assert bool(torch.isfinite(got).all()), f"{what}: not finite"
        e = rel_l2(got, want)
        assert e <= tol, f"{what}: rel-L2 {e:.3g} against the plain-allocation call (tolerance {tol})"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- conv, data gradient, wgrad, wgrad_bias, colsum -----------------------------------------------------------------------------------
CONV_CASES = [
    # (B, Cin, N, W, H, taps, stride, mode, pad)
    (3, 48, 32, 8, 4, 9, 1, 0, 0),          # direct fast
    (2, 5, 32, 16, 8, 9, 1, 0, 0),          # direct, Cin % 16 != 0
    (5, 128, 512, 1, 1, 1, 1, 0, 0),        # Linear
    (2, 32, 64, 16, 8, 9, 1, 0, 0),         # lds <32, 64>, split K
    (2, 96, 40, 8, 4, 1, 1, 0, 0),          # N = 40
    (2, 64, 64, 16, 8, 9, 1, 0, 0),         # lds <64, 64> split / wgrad2<9> partials + reduce
    (2, 512, 128, 16, 4, 1, 1, 0, 0),       # wgrad2<1>, adds into dw
    (2, 64, 64, 16, 8, 9, 2, 0, 0),         # stride 2 and its mode-2 data gradient
    (2, 64, 64, 8, 4, 9, 1, 1, 0),          # nearest x2 with sum2x2
    (4, 64, 128, 256, 16, 9, 1, 0, 0),      # halo <64>
    (1, 64, 2, 8, 64, 9, 1, 0, 0),          # the VAE's conv_out, N = 2: output rows of 8 bytes
    (1, 2, 64, 8, 64, 9, 1, 0, 0),          # the VAE's conv_in, Cin = 2
    (3, 32, 32, 6, 8, 9, 2, 0, 1),          # end-only padding
    (1, 16, 16, 2, 2, 9, 2, 0, 1),          # end-only padding, one output pixel
]


def _conv_ref(case):
    B, Cin, N, W, H, taps, stride, md, pad = case
    k = 3 if taps == 9 else 1
    x = int_grid((B, Cin, W, H), 201)
    w = int_grid((N, Cin, k, k), 202, -4, 4, exp=-5)
    bias, row = int_grid((N,), 203, -64, 64, exp=-5), int_grid((B, N), 204, -64, 64, exp=-5)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    if pad:
        y0 = o_ops.downsample_vae(x64, w64, bias.double())
    else:
        xin = F.interpolate(x64, scale_factor=2.0, mode="nearest") if md == 1 else x64
        y0 = o_ops.circ_conv2d(xin, w64, bias.double(), stride, 1 if taps == 9 else 0)
    res = int_grid(y0.shape, 206)
    pre_y = int_grid(y0.shape, 207, -100, 100)
    pre_dw = int_grid(w.shape, 208, -100, 100)
    pre_tot, pre_rows = int_grid((N,), 209, -100, 100), int_grid((B, N), 210, -100, 100)
    y = y0 + row.double()[:, :, None, None] + res.double()
    dy = int_grid(y0.shape, 205)
    y.backward(dy.double())
    P = B * y0.shape[2] * y0.shape[3]
    assert_exact_bound(U, (Cin * taps * 4, amax(x) * amax(w)), (3, amax(bias, row, res)), (1, amax(pre_y)))
    assert_exact_bound(U, (N * taps * 4, amax(dy) * amax(w)), (1, amax(pre_y)))               # data gradient (x 4: sum2x2)
    assert_exact_bound(1.0, (P, amax(dy) * amax(x)), (1, amax(pre_dw, pre_tot, pre_rows)))    # dw, rows, total
    return dict(x=x, w=w, bias=bias, row=row, res=res, dy=dy, pre_y=pre_y, pre_dw=pre_dw, pre_tot=pre_tot, pre_rows=pre_rows,
                y=y.detach(), dx=x64.grad, dw=w64.grad)


@residues
@both_modes
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_family_placed(case, det, r):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, taps, stride, md, pad = case
    o = REFS.get(case, lambda: _conv_ref(case))
    what = f"{case} {'deterministic' if det else 'default'} residue {r}"
    wn = ("n", "cin", "i", "j")
    Wo, Ho = o["y"].shape[2], o["y"].shape[3]
    nan = float("nan")
    wide = torch.full((B, N + 4), nan)                  # the row term as a column slice; a kernel that reads the other columns shows
    wide[:, 4:] = o["row"]
    with mode(det):
        wf, wt = T.pack_weights(o["w"].to(DEV), taps)
        act = p_in(x=cl(o["x"]), dy=cl(o["dy"]), res=cl(o["res"]), wide=wide)
        ops = place({"wf": wf, "wt": wt}, GUARD, "in", device=DEV)
        par = p_in(r, bias=o["bias"])
        ins = (act, ops, par)
        rowadd = act["wide"][:, 4:]
        # forward: bias + row + residual, into an output nobody wrote before
        out = p_out(y=(B, Wo, Ho, N))
        T.conv(act["x"], ops["wf"], N, taps, stride, md, bias=par["bias"], rowadd=rowadd, res=act["res"], out=out["y"], pad=pad)
        done("conv " + what, out, *ins)
        exact(nchw(out["y"]), o["y"], "conv " + what)
        # ... and added to a pre-filled output
        acc = p_acc(y=cl(o["pre_y"]))
        T.conv(act["x"], ops["wf"], N, taps, stride, md, bias=par["bias"], rowadd=rowadd, res=act["res"], out=acc["y"], accumulate=True,
               pad=pad)
        done("conv accumulate " + what, acc, *ins)
        exact(nchw(acc["y"]), o["y"] + o["pre_y"].double(), "conv accumulate " + what)
        # data gradient
        if md == 1:
            full = p_out(du=(B, Wo, Ho, Cin))
            T.conv(act["dy"], ops["wt"], Cin, taps, 1, 0, out=full["du"])
            dxo = p_out(dx=(B, W, H, Cin))
            call("rldm_train_sum2x2", full["du"], B, W, H, Cin, dxo["dx"])
            done("data gradient " + what, full, dxo, *ins)
        else:
            dxo = p_out(dx=(B, W, H, Cin))
            T.conv(act["dy"], ops["wt"], Cin, taps, 1, 2 if stride == 2 else 0, out=dxo["dx"], pad=pad)
            done("data gradient " + what, dxo, *ins)
        exact(nchw(dxo["dx"]), o["dx"], "data gradient " + what)
        dxa = p_acc(dx=cl(int_grid(o["x"].shape, 211, -100, 100)))
        if md != 1:
            T.conv(act["dy"], ops["wt"], Cin, taps, 1, 2 if stride == 2 else 0, out=dxa["dx"], accumulate=True, pad=pad)
            done("data gradient accumulate " + what, dxa, *ins)
            exact(nchw(dxa["dx"]), o["dx"] + int_grid(o["x"].shape, 211, -100, 100).double(), "data gradient accumulate " + what)
        # weight gradient into a pre-filled dw
        g = p_acc(r, dw=o["pre_dw"])
        T.wgrad(act["dy"], act["x"], g["dw"], taps, stride, md, pad=pad)
        done("wgrad " + what, g, *ins)
        exact(g["dw"], o["pre_dw"].double() + o["dw"], "wgrad " + what, wn)
        # with the bias / row sums of the same pass: rows as a column slice of a pre-filled matrix
        g = p_acc(r, dw=o["pre_dw"], total=o["pre_tot"])
        rw = torch.full((B, N + 4), 7.0)
        rw[:, 4:] = o["pre_rows"]
        rows = p_acc(rows=rw)
        T.wgrad_bias(act["dy"], act["x"], g["dw"], taps, stride, md, rows=rows["rows"][:, 4:], total=g["total"], rows_accumulate=True, pad=pad)
        done("wgrad_bias " + what, g, rows, *ins)
        exact(g["dw"], o["pre_dw"].double() + o["dw"], "wgrad_bias dw " + what, wn)
        exact(g["total"], o["pre_tot"] + o["dy"].sum((0, 2, 3)), "wgrad_bias total " + what)
        exact(rows["rows"][:, 4:], o["pre_rows"] + o["dy"].sum((2, 3)), "wgrad_bias rows " + what)
        assert float((rows["rows"][:, :4] - 7.0).abs().max()) == 0, "wgrad_bias wrote the columns beside its rows " + what
        # column sums alone: rows written (not added), total added
        g = p_acc(r, total=o["pre_tot"])
        ro = p_out(rows=(B, N))
        T.colsum(act["dy"], rows=ro["rows"], total=g["total"])
        done("colsum " + what, g, ro, *ins)
        exact(ro["rows"], o["dy"].sum((2, 3)), "colsum rows " + what)
        exact(g["total"], o["pre_tot"] + o["dy"].sum((0, 2, 3)), "colsum total " + what)


# ---- two split-K convs back to back from one ZeroArena ---------------------------------------------------------------------------------
ARENA_CONVS = [
    # (B, Cin, N, W, H): 3x3; P = B W H >= 64 output pixels and P N no multiple of 4
    (1, 64, 33, 13, 5),                     # 65 pixels x 33 channels = 2145 floats: 3 rounding floats behind it
    (3, 64, 34, 5, 5),                      # 75 x 34 = 2550: 2 rounding floats
]


def test_two_split_k_convs_share_one_arena():
    """ZeroArena.take packs the slices at a 16-byte granule and a split-K launch only ADDS into its slice: a store past one conv's output
    is an additive error in the next conv's.  The arena's buffer is a placed view (pre-zeroed, as begin() leaves it)."""
    from rangeldm_amd import train_ops as T
    ncap = 8192
    buf = p_acc(arena=torch.zeros(ncap))
    arena = T.ZeroArena(torch.device(DEV), ncap * 4)
    arena.buf = buf["arena"]
    T.set_zero_arena(arena)
    ys, refs, ends = [], [], []
    try:
        for i, (B, Cin, N, W, H) in enumerate(ARENA_CONVS):
            x = int_grid((B, Cin, W, H), 700 + i)
            w = int_grid((N, Cin, 3, 3), 710 + i, -4, 4, exp=-5)
            bias = int_grid((N,), 720 + i, -64, 64, exp=-5)
            assert_exact_bound(U, (Cin * 9, amax(x) * amax(w)), (1, amax(bias)))
            assert (B * W * H * N) % 4 != 0
            d = T.conv_desc(torch.empty(B, W, H, Cin), N, 9)
            assert _lib.lib().rldm_train_conv_splits(C.byref(d), 0) > 1, f"{(B, Cin, N, W, H)} is no split-K launch"
            wf, _ = T.pack_weights(w.to(DEV), 9, want_transposed=False)
            ins = p_in(x=cl(x), bias=bias)
            pos = arena.pos
            y = T.conv(ins["x"], wf, N, 9, bias=ins["bias"])
            assert y.data_ptr() == buf["arena"].data_ptr() + 4 * pos, "the conv did not draw its output from the arena"
            ys.append((y, ins))
            refs.append(o_ops.circ_conv2d(x.double(), w.double(), bias.double()))
            ends.append((pos + y.numel(), arena.pos))
    finally:
        T.set_zero_arena(None)
    done("arena", buf, *[i for _, i in ys])
    for (y, _), ref, case in zip(ys, refs, ARENA_CONVS):
        exact(nchw(y), ref, f"split-K conv in the arena {case}")
    flat = buf["arena"].cpu()
    for (e0, e1), case in zip(ends, ARENA_CONVS):
        assert 1 <= e1 - e0 <= 3 and not bool(flat[e0:e1].any()), f"the rounding floats behind {case} are no longer zero: {flat[e0:e1]}"
    assert not bool(flat[arena.pos:].any()), "the arena beyond pos is no longer zero"


# ---- grouped weight gradients: every layer's dw / total as consecutive views of one flat buffer -----------------------------------------
@residues
@both_modes
def test_grouped_wgrad_into_one_flat_buffer(det, r):
    from rangeldm_amd import train_ops as T
    layers = [l for l in GROUP_LAYERS if l[4] <= 8]
    assert len(layers) >= 5

    def build():
        out, sizes = [], []
        for i, (B, Cin, N, W, H, taps, md) in enumerate(layers):
            k = 3 if taps == 9 else 1
            x = int_grid((B, Cin, W, H), 300 + i)
            Wo, Ho = (W, H) if md == 0 else (2 * W, 2 * H)
            dy = int_grid((B, N, Wo, Ho), 320 + i)
            xin = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if md == 1 else x.double()
            w64 = torch.zeros(N, Cin, k, k, dtype=torch.float64, requires_grad=True)
            o_ops.circ_conv2d(xin, w64, None, 1, 1 if taps == 9 else 0).backward(dy.double())
            assert_exact_bound(1.0, (B * Wo * Ho * (4 if md == 1 else 1), 9.0), (1, 100.0))
            out.append((x, dy, w64.grad))
            sizes += [N * Cin * k * k, N]                        # weight, bias: the trainers' order
        return out, sizes
    data, sizes = REFS.get("grouped", build)
    pre = int_grid((sum(sizes),), 340, -100, 100)
    flat = p_acc(r, grads=pre)                                  # ONE view: no guards between the layers
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    acts, views = [], []
    with mode(det):
        T.wgrad_group(True)
        try:
            for i, ((B, Cin, N, W, H, taps, md), (x, dy, _)) in enumerate(zip(layers, data)):
                k = 3 if taps == 9 else 1
                a = p_in(dy=cl(dy), x=cl(x))
                dw = flat["grads"][offs[2 * i]:offs[2 * i + 1]].view(N, Cin, k, k)
                tot = flat["grads"][offs[2 * i + 1]:offs[2 * i + 2]]
                rows = p_out(rows=(B, N))
                T.wgrad_bias(a["dy"], a["x"], dw, taps, 1, md, rows=rows["rows"], total=tot)
                acts.append(a), views.append((dw, tot, rows))
            assert T.wgrad_group_pending() == len(layers)
            T.wgrad_group_flush()
        finally:
            T.wgrad_group(False)
    done(f"grouped wgrad det={det}", flat, *acts, *[v[2] for v in views])
    for i, (case, (x, dy, g), (dw, tot, rows)) in enumerate(zip(layers, data, views)):
        exact(dw, pre[offs[2 * i]:offs[2 * i + 1]].view(dw.shape).double() + g, f"grouped dw {case}", ("n", "cin", "i", "j"))
        exact(tot, pre[offs[2 * i + 1]:offs[2 * i + 2]] + dy.sum((0, 2, 3)), f"grouped total {case}")
        exact(rows["rows"], dy.sum((2, 3)), f"grouped rows {case}")


# ---- the deferred reduction --------------------------------------------------------------------------------------------------------
@residues
@both_modes
@pytest.mark.parametrize("rider", ["split-k", "flush"])
def test_deferred_reduction_placed(rider, det, r):
    """(deterministic mode: the rider's conv is never split; the reduction rides on its single plane all the same)"""
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H = WG
    x, dy = int_grid((B, Cin, W, H), 401), int_grid((B, N, W, H), 402)
    w64 = torch.zeros(N, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    o_ops.circ_conv2d(x.double(), w64, None).backward(dy.double())
    pre = int_grid((N, Cin, 3, 3), 403, -100, 100)
    assert_exact_bound(1.0, (B * W * H, 9.0), (1, amax(pre)))
    a = p_in(dy=cl(dy), x=cl(x))
    g = p_acc(r, dw=pre)
    bufs, y, ref = [a, g], None, None
    prev = T.deterministic_enabled()
    T.deterministic(det)
    T.defer_reduce(True)
    try:
        T.wgrad(a["dy"], a["x"], g["dw"], 9)
        assert T.reduce_pending()
        if RIDERS[rider] is None:
            T.flush_reduce()
        else:
            cb, cc, cn, cw, chh, k = RIDERS[rider]
            cx, cwt = int_grid((cb, cc, cw, chh), 404), int_grid((cn, cc, 2 * k + 1, 2 * k + 1), 405, -4, 4, exp=-5)
            cbias = int_grid((cn,), 406, -64, 64, exp=-5)
            assert_exact_bound(U, (cc * (2 * k + 1) ** 2, amax(cx) * amax(cwt)), (1, amax(cbias)))
            wf, _ = T.pack_weights(cwt.to(DEV), 9 if k else 1, want_transposed=False)
            ref = o_ops.circ_conv2d(cx.double(), cwt.double(), cbias.double(), 1, k)
            ci, cp, y = p_in(x=cl(cx)), p_in(r, bias=cbias), p_out(y=(cb, cw, chh, cn))
            T.conv(ci["x"], wf, cn, 9 if k else 1, bias=cp["bias"], out=y["y"])
            bufs += [ci, cp, y]
        assert not T.reduce_pending(), "the reduction is still pending"
    finally:
        T.defer_reduce(False)
        T.deterministic(prev)
    done(f"deferred reduction ({rider}) det={det}", *bufs)
    exact(g["dw"], pre.double() + w64.grad, f"deferred reduction ({rider})", ("n", "cin", "i", "j"))
    if y is not None:
        exact(nchw(y["y"]), ref, f"conv carrying the reduction ({rider})")


# ---- conv_fused / wgrad_fused with gamma = 0 -----------------------------------------------------------------------------------------
def _fused_ref(case):
    B, C0, C1, N, W, H, taps = case
    k = 3 if taps == 9 else 1
    Cin = C0 + C1
    x = int_grid((B, Cin, W, H), 601)
    idx = torch.randint(0, len(H_GRID), (Cin,), generator=torch.Generator().manual_seed(602))
    h = torch.tensor(H_GRID, dtype=torch.float32)[idx]
    beta = silu_targets(h)
    w = int_grid((N, Cin, k, k), 603, -4, 4, exp=-5)
    bias, row, res = int_grid((N,), 604, -64, 64, exp=-5), int_grid((B, N), 605, -64, 64, exp=-5), int_grid((B, N, W, H), 606)
    dy = int_grid((B, N, W, H), 607)
    pre_dw = int_grid(w.shape, 608, -100, 100)
    assert_exact_bound(2.0 ** -8, (Cin * taps, 2 * amax(w)), (1, amax(bias)), (1, amax(row)), (1, amax(res)))
    assert_exact_bound(2.0 ** -3, (B * W * H, 2 * amax(dy)), (1, amax(pre_dw)))
    hm = h.double()[None, :, None, None].expand(B, -1, W, H).contiguous()
    w64 = w.double().requires_grad_()
    ref = o_ops.circ_conv2d(hm, w64, bias.double(), 1, 1 if taps == 9 else 0) + row.double()[:, :, None, None] + res.double()
    ref.backward(dy.double())
    return dict(x=x, beta=beta, w=w, bias=bias, row=row, res=res, dy=dy, pre_dw=pre_dw, y=ref.detach(), dw=w64.grad)


@residues
@both_modes
@pytest.mark.parametrize("case", [(8, 256, 0, 256, 32, 2, 9), (2, 96, 0, 64, 32, 4, 9), (3, 64, 64, 64, 64, 2, 9)],
                         ids=lambda c: "x".join(map(str, c)))
def test_fused_gamma0_placed(case, det, r):
    """y and dw are exact (gamma = 0: act(GN(x)) is act(beta) per channel).  The statistics outputs are sums of squares and of products
    with xhat, which the grids do not make exact: cs_out / gs_out / dz are compared with the same call on plain allocations -- bit for
    bit in the deterministic mode; the default mode adds them with atomics: tests/test_train_ops.py's 1e-4 for the statistics, TOL_MM
    for dz."""
    from rangeldm_amd import train_ops as T
    B, C0, C1, N, W, H, taps = case
    Cin = C0 + C1
    o = REFS.get(("fused", case), lambda: _fused_ref(case))
    what = f"{case} {'deterministic' if det else 'default'} residue {r}"
    xh = cl(o["x"])
    parts = {"x0": xh[..., :C0].contiguous()}
    if C1:
        parts["x1"] = xh[..., C0:].contiguous()
    with mode(det):
        wf, wt = T.pack_weights(o["w"].to(DEV), taps)
        plain = [T.Src(t.to(DEV)) for t in parts.values()]
        for s in plain:
            s.cs = T.chan_stats(s.t)
        act = p_in(res=cl(o["res"]), row=o["row"], dy=cl(o["dy"]), **parts)
        stat = p_in(**{f"cs{i}": s.cs.cpu() for i, s in enumerate(plain)})
        par = p_in(r, gamma=torch.zeros(Cin), beta=o["beta"], bias=o["bias"])
        ops = place({"wf": wf, "wt": wt}, GUARD, "in", device=DEV)
        ins = (act, stat, par, ops)
        srcs = [T.Src(act[n], stat[f"cs{i}"]) for i, n in enumerate(parts)]
        gn = T.GN(par["gamma"], par["beta"], True, 32, 1e-5)
        gn0 = T.GN(torch.zeros(Cin, device=DEV), o["beta"].to(DEV), True, 32, 1e-5)
        d = T._desc_srcs(srcs, N, taps, 1, 0)

        def fused(srcs_, w_, gn_, bias_, row_, res_, y_, cs_out=None, gsrcs=None, ggn=None, gs_out=None, desc=d):
            f, keep = T._fuse(srcs_, gn_, cs_out, gsrcs, ggn, gs_out)
            call("rldm_train_conv_fused", C.byref(desc), C.byref(f), srcs_[0].t, w_, bias_, row_, 0 if row_ is None else row_.stride(0),
                 res_, y_, 0)
        # forward with the output's statistics
        out, st = p_out(y=(B, W, H, N)), p_acc(cs_out=torch.zeros(B, N, 2))
        fused(srcs, ops["wf"], gn, par["bias"], act["row"], act["res"], out["y"], cs_out=st["cs_out"])
        done("conv_fused + statistics " + what, out, st, *ins)
        exact(nchw(out["y"]), o["y"], "conv_fused + statistics " + what)
        y0, cs0 = T.conv_fused(plain, wf, N, taps, gn=gn0, bias=o["bias"].to(DEV), rowadd=o["row"].to(DEV), res=cl(o["res"]).to(DEV),
                               want_stats=True)
        same(st["cs_out"], cs0, "cs_out " + what, None if det else 1e-4)
        # ... and without (the register epilogue)
        out = p_out(y=(B, W, H, N))
        fused(srcs, ops["wf"], gn, par["bias"], act["row"], act["res"], out["y"])
        done("conv_fused " + what, out, *ins)
        exact(nchw(out["y"]), o["y"], "conv_fused " + what)
        # the data-gradient form: dz and gs_out
        dsrc = [T.Src(act["dy"])]
        if T.conv_fused_ok(dsrc, Cin, taps, gsrcs=srcs, ggn=gn):
            dzo, gs = p_out(dz=(B, W, H, Cin)), p_acc(gs_out=torch.zeros(B, Cin, 2))
            fused(dsrc, ops["wt"], None, None, None, None, dzo["dz"], gsrcs=srcs, ggn=gn, gs_out=gs["gs_out"],
                  desc=T._desc_srcs(dsrc, Cin, taps, 1, 0))
            done("conv_fused data gradient " + what, dzo, gs, *ins)
            dz0, gs0 = T.conv_fused([T.Src(cl(o["dy"]).to(DEV))], wt, Cin, taps, gsrcs=plain, ggn=gn0)
            same(dzo["dz"], dz0, "dz " + what, None if det else TOL_MM)
            same(gs["gs_out"], gs0, "gs_out " + what, None if det else 1e-4)
        if T.wgrad_fused_ok(srcs, N, taps, gn=gn):
            g = p_acc(r, dw=o["pre_dw"])
            T.wgrad_fused(act["dy"], srcs, g["dw"], taps, gn=gn)
            done("wgrad_fused " + what, g, *ins)
            exact(g["dw"], o["pre_dw"].double() + o["dw"], "wgrad_fused " + what, ("n", "cin", "i", "j"))
            g = p_acc(r, dw=o["pre_dw"])
            T.wgrad_group(True)
            try:
                T.wgrad_fused(act["dy"], srcs, g["dw"], taps, gn=gn)
                assert T.wgrad_group_pending() == 1
            finally:
                T.wgrad_group(False)
            done("grouped wgrad_fused " + what, g, *ins)
            exact(g["dw"], o["pre_dw"].double() + o["dw"], "grouped wgrad_fused " + what, ("n", "cin", "i", "j"))


# ---- rows-wise Linear kernels -----------------------------------------------------------------------------------------------------
@residues
@both_modes
@pytest.mark.parametrize("B,K,N", [(3, 40, 24), (8, 512, 4352)])
def test_linear_rows_placed(B, K, N, det, r):
    from rangeldm_amd import train_ops as T
    x = int_grid((B, K), 501)
    w = int_grid((N, K), 502, -4, 4, exp=-5)
    bias = int_grid((N,), 503, -64, 64, exp=-5)
    dy = int_grid((B, N), 504)
    pre_y, pre_dw, pre_db = int_grid((B, N), 505, -100, 100), int_grid((N, K), 506, -100, 100), int_grid((N,), 507, -100, 100)
    assert_exact_bound(U, (K, amax(x) * amax(w)), (1, amax(bias)), (1, amax(pre_y)))
    assert_exact_bound(U, (N, amax(dy) * amax(w)))
    assert_exact_bound(1.0, (B, amax(dy) * amax(x)), (1, amax(pre_dw, pre_db)))
    what = f"{(B, K, N)} det={det} residue {r}"
    wide = torch.full((B, K + 8), float("nan"))
    wide[:, 4:4 + K] = x
    y_ref = x.double() @ w.double().T + bias.double()
    with mode(det):
        wf, wt = T.pack_weights(w.to(DEV), 1)
        act, ops, par = p_in(wide=wide, dy=dy), place({"wf": wf, "wt": wt}, GUARD, "in", device=DEV), p_in(r, bias=bias)
        ins = (act, ops, par)
        xs = act["wide"][:, 4:4 + K]
        out = p_out(y=(B, N))
        T.linear_rows(xs, ops["wf"], N, bias=par["bias"], out=out["y"])
        done("linear_rows " + what, out, *ins)
        exact(out["y"], y_ref, "linear_rows " + what)
        acc = p_acc(y=pre_y)
        T.linear_rows(xs, ops["wf"], N, bias=par["bias"], out=acc["y"], accumulate=True)
        done("linear_rows accumulate " + what, acc, *ins)
        exact(acc["y"], y_ref + pre_y.double(), "linear_rows accumulate " + what)
        dxo = p_out(dx=(B, K))
        T.linear_rows(act["dy"], ops["wt"], K, out=dxo["dx"])
        done("linear_rows data gradient " + what, dxo, *ins)
        exact(dxo["dx"], dy.double() @ w.double(), "linear_rows data gradient " + what)
        g = p_acc(r, dw=pre_dw, dbias=pre_db)
        T.linear_rows_wgrad(act["dy"], xs, g["dw"], g["dbias"])
        done("linear_rows_wgrad " + what, g, *ins)
        exact(g["dw"], pre_dw.double() + dy.double().T @ x.double(), "linear_rows_wgrad " + what)
        exact(g["dbias"], pre_db + dy.sum(0), "linear_rows_wgrad bias " + what)


# ---- elementwise ----------------------------------------------------------------------------------------------------------------
@both_modes
def test_elementwise_placed(det):
    shp = (3, 7, 11, 5)                                         # 1155 elements: no multiple of 4 or of 256
    a, b = int_grid(shp, 801), int_grid(shp, 802)
    with mode(det):
        ins, out = p_in(a=a, b=b), p_out(y=shp)
        call("rldm_train_add", ins["a"], ins["b"], out["y"], a.numel())
        done("add", out, ins)
        exact(out["y"], a + b, "add")
        # copy_channels: (src channels, src offset, dst channels, dst offset, ncopy); the vector route needs every one a multiple of 4
        for sc, so, dc, do, nc in ((8, 4, 12, 4, 4), (7, 2, 9, 1, 3), (8, 4, 12, 4, 3), (8, 2, 12, 4, 4), (8, 4, 10, 4, 4)):
            for accumulate in (False, True):
                src = int_grid((3, 7, 11, sc), 803)
                pre = int_grid((3, 7, 11, dc), 804) + 1000.0            # never equal to a copied value
                si, d = p_in(src=src), p_acc(dst=pre)
                call("rldm_train_copy_channels", si["src"], sc, so, d["dst"], dc, do, nc, 3 * 7 * 11, 1 if accumulate else 0)
                what = f"copy_channels {(sc, so, dc, do, nc)} accumulate={accumulate}"
                done(what, d, si)
                want = pre.clone()
                want[..., do:do + nc] = src[..., so:so + nc] + (pre[..., do:do + nc] if accumulate else 0)
                exact(d["dst"], want, what)
        du = int_grid((2, 6, 10, 5), 805)
        ins, out = p_in(du=du), p_out(dx=(2, 3, 5, 5))
        call("rldm_train_sum2x2", ins["du"], 2, 3, 5, 5, out["dx"])
        done("sum2x2", out, ins)
        exact(out["dx"], du.view(2, 3, 2, 5, 2, 5).sum((2, 4)), "sum2x2")
        x = int_grid((2, 4, 7, 3), 806)
        pe = torch.zeros(2, 1, 7, 3)
        pe[:, :, 0, :] = 1
        for pos in (False, True):
            cch = 4 + (1 if pos else 0)
            ins, out = p_in(x=x), p_out(y=(2, 7, 3, cch))
            call("rldm_train_pack_input", ins["x"], 2, 4, 7, 3, 1 if pos else 0, out["y"])
            done(f"pack_input pos={pos}", out, ins)
            want = cl(torch.cat([x, pe], 1) if pos else x)
            exact(out["y"], want, f"pack_input pos={pos}")
            ins, out = p_in(y=want), p_out(x=(2, cch, 7, 3))
            call("rldm_train_unpack_output", ins["y"], 2, cch, 7, 3, out["x"])
            done(f"unpack_output C={cch}", out, ins)
            exact(out["x"], want.permute(0, 3, 1, 2), f"unpack_output C={cch}")


# ---- pack_weights -----------------------------------------------------------------------------------------------------------------
@residues
@both_modes
@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("N", [2, 40])
@pytest.mark.parametrize("Cin", [5, 2, 48])
def test_pack_weights_placed(Cin, N, taps, det, r):
    k = 3 if taps == 9 else 1
    w = int_grid((N, Cin, k, k), 901, -4, 4, exp=-5)
    cp, npad = (Cin + 15) // 16 * 16, (N + 15) // 16 * 16
    with mode(det):
        ins = p_in(r, w=w)
        out = p_out(dtype=torch.bfloat16, wf=(N, taps, cp), wt=(Cin, taps, npad))
        call("rldm_train_pack_weights", ins["w"], N, Cin, taps, out["wf"], out["wt"])
        done(f"pack_weights {(N, Cin, taps)}", out, ins)
    wv = w.view(N, Cin, taps)
    wf = torch.zeros(N, taps, cp)
    wf[:, :, :Cin] = wv.permute(0, 2, 1)
    wt = torch.zeros(Cin, taps, npad)
    wt[:, :, :N] = wv.flip(2).permute(1, 2, 0)
    exact(out["wf"].float(), wf, f"pack_weights forward copy {(N, Cin, taps)} (pads are zeros)", ("n", "tap", "c"))
    exact(out["wt"].float(), wt, f"pack_weights transposed copy {(N, Cin, taps)} (pads are zeros)", ("c", "tap", "n"))


# ---- losses and reductions against their host restatements -------------------------------------------------------------------------
@both_modes
def test_losses_and_sums_placed(det):
    from rangeldm_amd import train_ops as T
    f64 = torch.float64
    with mode(det):
        # l1: tests/test_vae_training_gpu.py's shapes (two channels, 126 elements; four channels: the vector kernel)
        for shape, wc in (((3, 2, 7, 3), (1.0, 0.5)), ((1, 4, 7, 3), (1.5, 0.25, 3.0, 7.0))):
            B, Cc, W, H = shape
            g = torch.Generator().manual_seed(21)
            pred, target = torch.randn(B, W, H, Cc, generator=g), torch.randn(B, Cc, W, H, generator=g)
            ties = torch.rand(B, W, H, Cc, generator=g) < 0.1
            pred = torch.where(ties, target.permute(0, 2, 3, 1), pred).contiguous()
            loss_h, dpred_h, sums_h = T.l1_host(pred.numpy(), target.numpy(), wc)
            ins = p_in(pred=pred, target=target, wc=torch.tensor(wc))
            out, words = p_out(dpred=pred.shape), p_out(dtype=f64, out=(1 + Cc,))
            call("rldm_train_l1", ins["pred"], ins["target"], ins["wc"], B, Cc, W, H, out["dpred"], words["out"])
            done(f"l1 {shape}", out, words, ins)
            exact(out["dpred"], torch.from_numpy(dpred_h), f"l1 dpred {shape}")
            got = words["out"].cpu().numpy()
            if det:
                assert got[0] == float(loss_h) and np.array_equal(got[1:], sums_h), f"l1 {shape}"
            else:                                               # (fp64 atomics: tests/test_vae_training_gpu.py's 1e-12)
                assert abs(got[0] - float(loss_h)) <= 1e-12 * float(loss_h) and np.allclose(got[1:], sums_h, rtol=1e-12, atol=0)
        # mse, with and without sample weights
        pred, tgt, wts = rnd(3, 7, 5, 4, seed=6), rnd(3, 4, 7, 5, seed=7), torch.tensor([0.5, 1.0, 0.25])
        for wgt in (wts, None):
            ins = p_in(pred=pred, target=tgt, w=wts)
            out, words = p_out(dpred=pred.shape), p_out(dtype=f64, loss=(1,))
            call("rldm_train_mse", ins["pred"], ins["target"], ins["w"] if wgt is not None else None, 3, 4, 7, 5, out["dpred"], words["loss"])
            done("mse", out, words, ins)
            l0, dp0 = T.mse(pred.to(DEV), tgt.to(DEV), None if wgt is None else wts.to(DEV))
            same(out["dpred"], dp0, "mse dpred")
            host = float(T.mse_host(pred.numpy(), tgt.numpy(), None if wgt is None else wts.numpy()))
            got = float(words["loss"][0])
            assert got == host if det else abs(got - host) < 1e-6, ("mse", got, host)      # (tests/test_train_ops.py: 1e-6)
        # sqnorm: one block sweep, and more than 2048 blocks' worth
        for n in (10007, 600001):
            gvec = rnd(n, seed=8)
            ins, words = p_in(g=gvec), p_out(dtype=f64, out=(1,))
            call("rldm_train_sqnorm", ins["g"], n, words["out"])
            done(f"sqnorm {n}", words, ins)
            got, host = float(words["out"][0]), float(T.sqnorm_host(gvec.numpy()))
            assert got == host if det else abs(got - host) < 1e-6 * host, ("sqnorm", n, got, host)
        # colsum / chan_stats against their fixed-order statements (deterministic mode; the default mode: TOL_F32 / 3e-3 as
        # tests/test_train_ops.py states them)
        for shape in ((2, 5, 7, 36), (2, 20, 20, 6)):          # 16-byte loads (N % 4 == 0) / scalar loads, two slabs
            dy = rnd(*shape, seed=9)
            pre_r, pre_t = rnd(shape[0], shape[3], seed=10), rnd(shape[3], seed=11)
            ins, acc = p_in(dy=dy), p_acc(rows=pre_r, total=pre_t)
            T.colsum(ins["dy"], rows=acc["rows"], total=acc["total"], rows_accumulate=True)
            done(f"colsum {shape}", acc, ins)
            rows_h, tot_h = T.colsum_host(dy.numpy(), pre_r.numpy(), pre_t.numpy())
            if det:
                exact(acc["rows"], torch.from_numpy(rows_h), f"colsum rows {shape}")
                exact(acc["total"], torch.from_numpy(tot_h), f"colsum total {shape}")
            else:
                assert rel_l2(acc["rows"], torch.from_numpy(rows_h)) < 3e-3 and rel_l2(acc["total"], torch.from_numpy(tot_h)) < 3e-3


@both_modes
@pytest.mark.parametrize("shape", [(2, 7, 11, 36), (1, 64, 64, 8)], ids=["npix77", "npix4096"])
def test_chan_stats_placed(shape, det):
    """npix = 77 with 36 channels; npix >= 4096 takes the 256-pixel slab.  Deterministic: equals chan_stats_host; default (atomics):
    TOL_F32 against the plain-allocation call, as tests/test_train_ops.py gates chan_stats."""
    from rangeldm_amd import train_ops as T
    x = rnd(*shape, seed=12)
    B, Cc = shape[0], shape[3]
    with mode(det):
        ins, acc = p_in(x=x), p_acc(cs=torch.zeros(B, Cc, 2))
        call("rldm_train_chan_stats", ins["x"], B, shape[1] * shape[2], Cc, acc["cs"])
        done(f"chan_stats {shape}", acc, ins)
        if det:
            exact(acc["cs"], torch.from_numpy(T.chan_stats_host(x.numpy())), f"chan_stats {shape}")
        same(acc["cs"], T.chan_stats(x.to(DEV)), f"chan_stats {shape}", None if det else TOL_F32)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------
GN_CASES = [
    # (B, C, W, H, slab)
    (3, 32, 8, 4, False),               # 1 channel per group: the scalar kernels
    (2, 96, 8, 4, False),               # 3 channels per group
    (2, 64, 16, 8, False),              # 2 channels per group
    (1, 128, 4, 2, False),              # the fused vector kernel
    (2, 512, 4, 2, False),              # 16 channels per group
    (2, 128, 256, 16, True),            # the slab kernels (default mode only: the deterministic mode never takes them)
]


@residues
@pytest.mark.parametrize("B,Cc,W,H,slab,det", [c + (d,) for c in GN_CASES for d in MODES if not (c[4] and d)], ids=lambda v: str(v))
def test_group_norm_placed(B, Cc, W, H, slab, det, r):
    """Against the same calls on plain allocations.  Bit for bit, except where the default route meets in atomics: d gamma / d beta over
    more than one image, and everything behind the slab kernels' fp64 atomics -- tests/test_train_ops.py's TOL_F32 (forward) and 1e-4
    (gradients)."""
    from rangeldm_amd import train_ops as T
    x, dy = cl(rnd(B, Cc, W, H, seed=1) * 2 + 0.5), cl(rnd(B, Cc, W, H, seed=4))
    gam, bet = 1 + 0.3 * rnd(Cc, seed=2), 0.2 * rnd(Cc, seed=3)
    pre_g, pre_b, pre_dx = int_grid((Cc,), 5), int_grid((Cc,), 6), cl(int_grid((B, Cc, W, H), 7))
    what = f"{(B, Cc, W, H)} det={det} residue {r}"
    t_fwd, t_dx = (TOL_F32, 1e-4) if slab else (None, None)
    t_par = None if (det or B == 1) else 1e-4
    with mode(det):
        xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), gam.to(DEV), bet.to(DEV)
        y0, st0 = T.gn_forward(xd, gd, bd, 32, 1e-5, True)
        dg0, db0 = pre_g.to(DEV), pre_b.to(DEV)
        dx0 = T.gn_backward(xd, dyd, st0, gd, bd, 32, True, dg0, db0)
        dg1, db1 = pre_g.to(DEV), pre_b.to(DEV)
        dx1 = T.gn_backward(xd, dyd, st0, gd, bd, 32, True, dg1, db1, dx=pre_dx.to(DEV), accumulate=True)
        act, par = p_in(x=x, dy=dy), p_in(r, gamma=gam, beta=bet)
        out = p_out(y=x.shape, stats=(B, 32, 2))
        call("rldm_train_gn_forward", act["x"], B, W * H, Cc, 32, 1e-5, par["gamma"], par["beta"], 1, out["stats"], out["y"])
        done("gn_forward " + what, out, act, par)
        same(out["y"], y0, "gn_forward y " + what, t_fwd)
        same(out["stats"], st0, "gn_forward stats " + what, t_fwd)
        st = p_in(stats=st0.cpu())
        for accumulate, dxref, dgref, dbref in ((False, dx0, dg0, db0), (True, dx1, dg1, db1)):
            o2 = p_out(scratch=(B, 32, 2)) if accumulate else p_out(scratch=(B, 32, 2), dx=x.shape)
            dxa = p_acc(dx=pre_dx) if accumulate else o2
            g = p_acc(r, dgamma=pre_g, dbeta=pre_b)
            call("rldm_train_gn_backward", act["x"], act["dy"], st["stats"], B, W * H, Cc, 32, par["gamma"], par["beta"], 1,
                 o2["scratch"], dxa["dx"], 1 if accumulate else 0, g["dgamma"], g["dbeta"])
            w2 = f"gn_backward accumulate={accumulate} " + what
            done(w2, o2, dxa, g, act, par, st)
            same(dxa["dx"], dxref, w2 + " dx", t_dx)
            same(g["dgamma"], dgref, w2 + " dgamma", 1e-4 if slab else t_par)
            same(g["dbeta"], dbref, w2 + " dbeta", 1e-4 if slab else t_par)


@residues
@both_modes
@pytest.mark.parametrize("B,C0,C1,W,H", [(2, 64, 0, 8, 8), (2, 64, 32, 8, 4), (3, 32, 0, 64, 64)],
                         ids=["one-source", "two-sources", "slab-doubles"])
def test_gn_backward_apply_placed(B, C0, C1, W, H, det, r):
    """One and two sources; B ceil(npix / 16) = 768 > 512: the slab doubles.  No atomics in this kernel: bit for bit in both modes."""
    from rangeldm_amd import train_ops as T
    Cc = C0 + C1
    parts = {"x0": rnd(B, W, H, C0, seed=1)}
    if C1:
        parts["x1"] = rnd(B, W, H, C1, seed=2)
    dz, gs, extra = rnd(B, W, H, Cc, seed=3), rnd(B, Cc, 2, seed=4), rnd(B, W, H, Cc, seed=5)
    gam = 1 + 0.3 * rnd(Cc, seed=6)
    pre_g, pre_b, pre1 = int_grid((Cc,), 7), int_grid((Cc,), 8), int_grid(tuple(parts[list(parts)[-1]].shape), 9)
    what = f"gn_backward_apply {(B, C0, C1, W, H)} det={det} residue {r}"
    with mode(det):
        plain = [T.Src(t.to(DEV)) for t in parts.values()]
        for s in plain:
            s.cs = T.chan_stats(s.t)
        gn0 = T.GN(gam.to(DEV), torch.zeros(Cc, device=DEV), True, 32, 1e-5)
        dg0, db0 = pre_g.to(DEV), pre_b.to(DEV)
        ref = T.gn_backward_apply(dz.to(DEV), plain, gs.to(DEV), gn0, dg0, db0, res=extra.to(DEV),
                                  dsts=([None, pre1.to(DEV)] if C1 else [pre1.to(DEV)]), accumulate=((False, True) if C1 else (True, False)))
        act = p_in(dz=dz, gs=gs, res=extra, **parts)
        stat = p_in(**{f"cs{i}": s.cs.cpu() for i, s in enumerate(plain)})
        par, g = p_in(r, gamma=gam), p_acc(r, dgamma=pre_g, dbeta=pre_b)
        srcs = [T.Src(act[n], stat[f"cs{i}"]) for i, n in enumerate(parts)]
        gn = T.GN(par["gamma"], None, True, 32, 1e-5)
        fresh, acc = (p_out(d0=parts["x0"].shape) if C1 else None), p_acc(d=pre1)
        dsts = [fresh["d0"], acc["d"]] if C1 else [acc["d"]]
        T.gn_backward_apply(act["dz"], srcs, act["gs"], gn, g["dgamma"], g["dbeta"], res=act["res"], dsts=dsts,
                            accumulate=((False, True) if C1 else (True, False)))
        done(what, acc, g, act, stat, par, *([fresh] if C1 else []))
        for i, (a, b) in enumerate(zip(dsts, ref)):
            same(a, b, f"{what} source {i}")
        same(g["dgamma"], dg0, what + " dgamma")
        same(g["dbeta"], db0, what + " dbeta")


# ---- attention -----------------------------------------------------------------------------------------------------------------------
@both_modes
@pytest.mark.parametrize("B,L,Cc", [(2, 4, 8), (1, 200, 16), (3, 16, 64)])
def test_attention_placed(B, L, Cc, det):
    """(1, 200, 16): rows past the last full tile.  train_attn.hip has no atomics: bit for bit against the plain-allocation calls."""
    from rangeldm_amd import train_ops as T
    q, k, v = (rnd(B, L, Cc, seed=s) * 1.5 for s in (1, 2, 3))
    dO = rnd(B, L, Cc, seed=4)
    nh = Cc // 8
    what = f"{(B, L, Cc)} det={det}"
    with mode(det):
        o0, lse0 = T.attention_forward(q.to(DEV), k.to(DEV), v.to(DEV))
        dq0, dk0, dv0 = T.attention_backward(q.to(DEV), k.to(DEV), v.to(DEV), o0, dO.to(DEV), lse0)
        ins = p_in(q=q, k=k, v=v, dO=dO, o=o0.cpu(), lse=lse0.cpu())
        out = p_out(o=(B, L, Cc), lse=(B, nh, L))
        call("rldm_train_attention_forward", ins["q"], ins["k"], ins["v"], B, L, Cc, out["o"], out["lse"])
        done("attention_forward " + what, out, ins)
        same(out["o"], o0, "attention o " + what)
        same(out["lse"], lse0, "attention lse " + what)
        g = p_out(delta=(B, nh, L), dq=(B, L, Cc), dk=(B, L, Cc), dv=(B, L, Cc))
        call("rldm_train_attention_backward", ins["q"], ins["k"], ins["v"], ins["o"], ins["dO"], ins["lse"], B, L, Cc, g["delta"], g["dq"],
             g["dk"], g["dv"])
        done("attention_backward " + what, g, ins)
        for n, ref in (("dq", dq0), ("dk", dk0), ("dv", dv0)):
            same(g[n], ref, f"attention {n} " + what)
        # the qkv forms: one (B, L, 3C) operand
        qkv = torch.cat([q, k, v], -1).contiguous()
        o1, lse1 = T.attention_qkv_forward(qkv.to(DEV))
        dqkv1 = T.attention_qkv_backward(qkv.to(DEV), o1, dO.to(DEV), lse1)
        ins = p_in(qkv=qkv, dO=dO, o=o1.cpu(), lse=lse1.cpu())
        out = p_out(o=(B, L, Cc), lse=(B, nh, L))
        call("rldm_train_attention_qkv_forward", ins["qkv"], B, L, Cc, out["o"], out["lse"])
        done("attention_qkv_forward " + what, out, ins)
        same(out["o"], o1, "attention qkv o " + what)
        same(out["lse"], lse1, "attention qkv lse " + what)
        g = p_out(delta=(B, nh, L), dqkv=(B, L, 3 * Cc))
        call("rldm_train_attention_qkv_backward", ins["qkv"], ins["o"], ins["dO"], ins["lse"], B, L, Cc, g["delta"], g["dqkv"])
        done("attention_qkv_backward " + what, g, ins)
        same(g["dqkv"], dqkv1, "attention dqkv " + what)


# ---- SiLU, time embedding, the posterior ---------------------------------------------------------------------------------------------
@both_modes
def test_silu_embedding_gaussian_placed(det):
    """Element-wise kernels: bit for bit against the plain-allocation calls; the fp64 kl word is a sum of atomics in the default mode
    (1e-12, as the loss words of l1)."""
    from rangeldm_amd import train_ops as T
    with mode(det):
        x, dy, pre = rnd(5, 77, seed=1), rnd(5, 77, seed=2), int_grid((5, 77), 3)          # 385 elements
        ins, out = p_in(x=x, dy=dy), p_out(y=x.shape, dx=x.shape)
        call("rldm_train_silu", ins["x"], None, out["y"], x.numel(), 0, 0)
        call("rldm_train_silu", ins["x"], ins["dy"], out["dx"], x.numel(), 1, 0)
        acc = p_acc(dx=pre)
        call("rldm_train_silu", ins["x"], ins["dy"], acc["dx"], x.numel(), 1, 1)
        done("silu", out, acc, ins)
        same(out["y"], T.silu(x.to(DEV)), "silu")
        same(out["dx"], T.silu_backward(x.to(DEV), dy.to(DEV)), "silu_backward")
        same(acc["dx"], T.silu_backward(x.to(DEV), dy.to(DEV), out=pre.to(DEV), accumulate=True), "silu_backward accumulate")
        t = torch.tensor([0, 3, 977, 500, 999]).to(DEV)
        out = p_out(emb=(5, 128))
        call("rldm_train_timestep_embedding", t, 5, 128, out["emb"])
        done("timestep_embedding", out)
        same(out["emb"], T.timestep_embedding(t, 128), "timestep_embedding")
        for B, Z, W, H in ((1, 3, 5, 7), (3, 4, 2, 8)):
            m, noise, dz = rnd(B, W, H, 2 * Z, seed=4), rnd(B, Z, W, H, seed=5), rnd(B, W, H, Z, seed=6)
            for nz in (noise, None):
                ins = p_in(m=m, noise=noise, dz=dz)
                out, word = p_out(z=(B, W, H, Z), dm=(B, W, H, 2 * Z)), p_out(dtype=torch.float64, kl=(1,))
                nd = ins["noise"] if nz is not None else None
                call("rldm_train_gaussian", ins["m"], nd, B, W, H, Z, out["z"], word["kl"])
                call("rldm_train_gaussian_backward", ins["m"], nd, ins["dz"], 0.25, B, W, H, Z, out["dm"])
                what = f"gaussian {(B, Z, W, H)} noise={nz is not None}"
                done(what, out, word, ins)
                n0 = None if nz is None else noise.to(DEV)
                z0, kl0 = T.gaussian(m.to(DEV), n0)
                same(out["z"], z0, what + " z")
                same(out["dm"], T.gaussian_backward(m.to(DEV), n0, dz.to(DEV), 0.25), what + " dmoments")
                got, ref = float(word["kl"][0]), float(kl0)
                assert got == ref if det else abs(got - ref) <= 1e-12 * abs(ref), (what, got, ref)
