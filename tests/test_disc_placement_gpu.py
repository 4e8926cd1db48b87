"""GPU: the discriminators' and the BEV terms' training kernels (rangeldm_amd/csrc/train_disc.hip, train_meta.hip, lidar.hip's
to_voxel_train / to_voxel_backward, and train_wgrad.hip's colsum and train.hip's pack_weights as the discriminators call them) on operands placed as
PatchDiscriminator and MetaKernelDiscriminator place them.

tests/test_train_placement_gpu.py's observation, for the kernels added since: a test that gives every operand its own torch tensor
cannot see a load or store one element past a view, because the caching allocator rounds every block up.  Both discriminators keep
their parameters and gradients in FlatParameters' flat buffers and hand views of them (`self.p[...]`, `self.g[...]`) straight to these
kernels, and every workspace of theirs is the caller's, sized by a *_workspace() function of the library.  Here every operand is a view
between guards (tests/hip_util.py: place / assert_placement, tested by tests/test_placement_host.py): inputs between quiet NaNs,
outputs between finite sentinels with a NaN pre-fill, accumulating outputs with integer pre-fill values that enter the reference, and
-- new with this file -- workspaces as kind "scratch": exactly the number of bytes the library asked for, between sentinels, the
interior not judged (a workspace may stay partly unwritten and its fp64 partials look like anything through an fp32 view).

Placements.  "r" below is DISC_RESIDUES: offset % 4 (floats) of every parameter / gradient view of the discriminators' flat buffers,
derived on the CPU by tests.hip_util.discriminator_residues (tests/test_placement_host.py asserts the list here equals it).  It is
[0, 2] today.  The PatchGAN's layouts give {0}.  The Meta-Kernel network, which vae/configs/kitti360.yaml selects, gives {0, 2}: its
first layer has C = 2 (mlp_coord.0.weight 6 floats, .0.bias 2, .2.weight 4, .2.bias 2), so main.0.mlp_coord.0.bias and EVERY view from
main.0.coov.weight to the end of the buffer -- all later MLP weights, every coov weight and bias, every BatchNorm gamma and beta, and all
of their gradients -- start 8 bytes into a 16-byte granule.  Activations, dy, saved tensors (BatchNorm's save, the layer's pe / src /
m), the packed bf16 weights and the workspaces are torch allocations: residue 0.

  op                                         placed                                                          residues     modes
  disc_conv / _conv_dgrad                    x, dy, wf, wt in; y, dx out                                     bias: r      both
  disc_wgrad (+ its colsum), 5 + 1 cases     dy, x in; dw, dbias acc; the workspace scratch (the sliced      dw, dbias:   both
                                             case: > 0 bytes); a second call accumulates                     r
  pack_weights, 16 taps                      w in; wf, wt bf16 out                                           w: r         both
  disc_bn_forward (training)                 x in; save, y out; the workspace scratch                        gamma, beta, both
                                                                                                             running
                                                                                                             mean / var
                                                                                                             (acc): r
  disc_bn_forward (eval)                     x in; save, y out                                               gamma, beta, both
                                                                                                             running
                                                                                                             statistics
                                                                                                             (in): r
  disc_bn_backward, with and without         x, dy, save in; dx out; the workspace scratch                   gamma, beta, both
    dgamma / dbeta                                                                                           dgamma,
                                                                                                             dbeta (acc):
                                                                                                             r
  disc_lrelu forward / backward              every operand                                                   0            both
  disc_hinge, disc_generator                 real, fake in; dreal, dfake out; out fp64 out; partials fp64    0            both
                                             scratch
  disc_adaptive_mix                          dnll, dg, the two fp64 squared norms in; dpred, d_weight out    0            both
  colsum, rows = nullptr                     dy in                                                           total (acc): both
                                                                                                             r
  meta_forward                               x, r, tables in; y, r_next, pe, m out (src: a plain int32       w1, b1, w2,  both
                                             tensor); the workspace scratch                                  b2, coov,
                                                                                                             bias: r
  meta_backward, its two partial forms       x, dy, tables, pe, m, dr_next in; dx, dr out; the workspace     w1, b1, w2,  both
                                             scratch                                                         coov (in),
                                                                                                             the six
                                                                                                             gradients
                                                                                                             (acc): r
  meta_range / _range_grad                   x in, r out; dr in, dx acc                                      0            both
  lidar_to_voxel_train / _backward           images (C = 2; C = 3 with a NaN channel 2), raw, dvoxel in;     0            default
                                             raw, voxel, cell_grad, dimages out                                           (no switch)

What the read-through of these kernels found, per operand class ("scalar" = 4-byte accesses only; nothing needed a fix):
  bias      dc_conv_kernel adds `p.bias[ch]` per output element; mk_gemm_kernel / mk_reduce_kernel `p.bias[n]`: scalar throughout
  weights   (fp32 masters) tr_pack_weights_kernel reads one element per thread; the Meta-Kernel layer reads w1 / b1 / w2 / b2 / coov
            through mk_load, mk_mask_kernel and the index map mk_at, one float at a time: scalar throughout.  The 16-byte loads of
            dc_conv_kernel (uint4 of wf / wt, float4 of FAST x rows) and of dc_load4 / tr_colsum_kernel (dy, x when N % 4 == 0) are on
            packed bf16 copies and activations: torch allocations, and G / dh inside the meta workspace, whose offsets are multiples of
            16 rows
  gamma,    dc_bn_partial_kernel<BWD>, dc_bn_apply_fwd / _bwd_kernel index [c]; the running statistics are read and written per
  beta,     channel by dc_bn_finish_fwd_kernel / dc_bn_eval_stats_kernel: scalar throughout
  running
  dw        dc_wgrad_kernel `out[idx] += acc[r]` (one slice) or stores to part[slice] and dc_wgrad_reduce_kernel `dw[e] += a`;
            mk_gemm_kernel / mk_reduce_kernel `*o = *o + v` through mk_at (dcoov's [c][t] order): scalar throughout
  dbias,    rldm_train_colsum with rows = nullptr: unsafeAtomicAdd of one float (default) or tr_colsum_finish_kernel's `total[c]`
  db1, db2  (deterministic): scalar
  dgamma,   dc_bn_finish_bwd_kernel `dgamma[c] += (float) s1`: scalar; no floating-point atomics in the BatchNorm kernels
  dbeta
  work-     rldm_train_disc_wgrad_workspace = slices N Cin 16 floats: dc_wgrad_kernel writes part[z][n][c][t], z < slices, nothing else;
  spaces    rldm_train_disc_bn_workspace = ceil(M / 256) C 2 doubles + 2 C floats: the partials, then coef (backward only);
            rldm_train_meta_workspace = (G | dh | dpe | part) with part the largest of the seven GEMMs' slices M N -- the forward's two
            ((R, C, C) and (P, N, 16 C)) and the backward's six ((P, 16 C, N), (N, 16 C, P), (C, C, R), (R, C, C), (C, 3, R), (R, 3, C)),
            all seven in mk_sizes; the forward uses the block from offset 0; hinge / generator partials = 3 / 1 x ceil(n / 256) doubles,
            written in the deterministic mode only.  Every formula covers its slice plan
  BEV       bev_splat_kernel, bev_finalize_train_kernel, bev_cell_grad_kernel, bev_pixel_grad_kernel: one element per access, channels
            0 and 1 of the image only (`im[n]`, `im[N + n]`): scalar throughout

Ops on integer grids must EQUAL the fp64 reference the op's own test builds (imported from there); the BatchNorm kernels, pack_weights
and the BEV backward are compared with the same call on plain torch allocations bit for bit; the BEV forward, which meets in fp32
atomics, under the per-cell bounds of tests/test_bev_training_gpu.py::test_forward_keeps_the_accumulators_and_to_voxels_bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd import discriminator as D
from rangeldm_amd import metakernel as MK
from tests import bev_util as BU
from tests.disc_util import mode
from tests.hip_util import GUARD, amax, assert_exact_bound, discriminator_residues, int_grid, place
from tests.meta_util import exact_layer_case
from tests.test_discriminator_gpu import CONV_CASES, _bn_case, _conv_reference, _logits
from tests.test_metakernel_gpu import LAYER_CASES
from tests.test_train_placement_gpu import DEV, both_modes, call, cl, done, exact, p_acc, p_in, p_out, same

pytestmark = pytest.mark.gpu
DISC_RESIDUES = sorted(set().union(*discriminator_residues().values()))
residues = pytest.mark.parametrize("r", DISC_RESIDUES, ids=lambda r: f"residue{r}")
F64 = torch.float64


def p_ws(dtype=torch.float32, **sizes):
    """caller-owned workspaces of exactly `sizes` elements each: kind "scratch", residue 0 (the wrappers allocate them with torch)"""
    return place({k: (int(v),) for k, v in sizes.items()}, GUARD, "scratch", device=DEV, dtype=dtype)


def ws_bytes(nbytes):
    """-> (Placement or None, pointer argument, byte count) for a workspace of exactly the bytes the library reported"""
    nbytes = int(nbytes)
    assert nbytes >= 0 and nbytes % 4 == 0, nbytes
    if nbytes == 0:
        return None, None, 0
    buf = p_ws(ws=nbytes // 4)
    assert buf["ws"].numel() * 4 == nbytes and buf["ws"].data_ptr() % 16 == 0
    return buf, buf["ws"], nbytes


def what_of(case, det, r):
    return f"{case} {'deterministic' if det else 'default'} residue {r}"


def tn(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the PatchGAN's 4x4 convs ---------------------------------------------------------------------------------------------------------
CONV_PLACED = [
    (1, 2, 64, 8, 64, 2),           # Cin = 2: the non-FAST gather
    (1, 512, 1, 3, 7, 1),           # N = 1: output rows of 4 bytes, dbias one float
    (1, 16, 16, 2, 2, 2),           # one output pixel, most taps in the padding
    (3, 32, 48, 7, 5, 2),           # odd everything; N = 48 leaves the second channel half of a tile empty
    (1, 16, 16, 4, 2, 2),
]
SLICED = (2, 2, 64, 64, 32, 2)      # tests/test_discriminator_gpu.py::test_conv4_weight_gradient_with_many_slices: several K slices
assert all(c in CONV_CASES for c in CONV_PLACED)


def _wgrad_placed(case, det, r, act, sliced):
    B, Cin, N, W, H, stride = case
    x, w, bias, dy, ref, dx_ref, dw_ref = _conv_reference(case)
    what = what_of(case, det, r)
    pre_dw, pre_db = int_grid(w.shape, 708, -100, 100), int_grid((N,), 709, -100, 100)
    P = B * ref.shape[2] * ref.shape[3]
    assert_exact_bound(1.0, (2 * P, amax(dy) * amax(x)), (1, amax(pre_dw, pre_db)))            # two calls on top of the pre-fill
    d = D.conv_desc((B, W, H, Cin), N, stride)
    nbytes = _lib.lib().rldm_train_disc_wgrad_workspace(C.byref(d))
    assert (nbytes > 0) == sliced, f"{case}: rldm_train_disc_wgrad_workspace = {nbytes}"
    ws, wsp, nbytes = ws_bytes(nbytes)
    bufs = [act] + ([ws] if ws is not None else [])
    wn = ("n", "cin", "i", "j")
    g = p_acc(r, dw=pre_dw, dbias=pre_db)
    call("rldm_train_disc_wgrad", C.byref(d), act["dy"], act["x"], g["dw"], g["dbias"], wsp, nbytes)
    done("wgrad " + what, g, *bufs)
    exact(g["dw"], pre_dw.double() + dw_ref, "weight gradient " + what, wn)
    exact(g["dbias"], pre_db.double() + dy.double().sum((0, 2, 3)), "bias sum " + what, ("n",))
    call("rldm_train_disc_wgrad", C.byref(d), act["dy"], act["x"], g["dw"], None, wsp, nbytes)
    done("wgrad, second call " + what, g, *bufs)
    exact(g["dw"], pre_dw.double() + 2 * dw_ref, "weight gradient, second call " + what, wn)
    exact(g["dbias"], pre_db.double() + dy.double().sum((0, 2, 3)), "bias sum after a call without dbias " + what, ("n",))


@residues
@both_modes
@pytest.mark.parametrize("case", CONV_PLACED, ids=lambda c: "x".join(map(str, c)))
def test_conv4_placed(case, det, r):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, stride = case
    x, w, bias, dy, ref, dx_ref, dw_ref = _conv_reference(case)
    what = what_of(case, det, r)
    Wo, Ho = ref.shape[2], ref.shape[3]
    d = D.conv_desc((B, W, H, Cin), N, stride)
    with mode(det):
        wf, wt = T.pack_weights(w.to(DEV), 16)
        act = p_in(x=cl(x), dy=cl(dy))
        ops = place({"wf": wf, "wt": wt}, GUARD, "in", device=DEV)
        par = p_in(r, bias=bias)
        ins = (act, ops, par)
        out = p_out(y=(B, Wo, Ho, N))
        call("rldm_train_disc_conv", C.byref(d), act["x"], ops["wf"], par["bias"], out["y"])
        done("conv " + what, out, *ins)
        exact(out["y"].permute(0, 3, 1, 2), ref, "conv " + what)
        out = p_out(y=(B, Wo, Ho, N))
        call("rldm_train_disc_conv", C.byref(d), act["x"], ops["wf"], None, out["y"])
        done("conv without bias " + what, out, *ins)
        exact(out["y"].permute(0, 3, 1, 2), ref - bias.double()[None, :, None, None], "conv without bias " + what)
        dxo = p_out(dx=(B, W, H, Cin))
        call("rldm_train_disc_conv_dgrad", C.byref(d), act["dy"], ops["wt"], dxo["dx"])
        done("data gradient " + what, dxo, *ins)
        exact(dxo["dx"].permute(0, 3, 1, 2), dx_ref, "data gradient " + what)
        _wgrad_placed(case, det, r, act, sliced=False)


@residues
@both_modes
def test_sliced_weight_gradient_placed(det, r):
    """rldm_train_disc_wgrad_workspace > 0: the partial planes go to a workspace of exactly that size, the reduction adds them to dw."""
    x, w, bias, dy = _conv_reference(SLICED)[:4]
    with mode(det):
        _wgrad_placed(SLICED, det, r, p_in(x=cl(x), dy=cl(dy)), sliced=True)


@residues
@both_modes
@pytest.mark.parametrize("N,Cin", [(64, 2), (1, 32), (48, 32)], ids=lambda v: str(v))
def test_pack_weights_16_taps_placed(N, Cin, det, r):
    """(tests/test_train_placement_gpu.py places 9 and 1 taps.)  The packed copies equal the plain call's bit for bit, pads included."""
    from rangeldm_amd import train_ops as T
    w = int_grid((N, Cin, 4, 4), 901, -4, 4, exp=-5)
    cp, npad = (Cin + 15) // 16 * 16, (N + 15) // 16 * 16
    with mode(det):
        wf0, wt0 = T.pack_weights(w.to(DEV), 16)
        ins = p_in(r, w=w)
        out = p_out(dtype=torch.bfloat16, wf=(N, 16, cp), wt=(Cin, 16, npad))
        call("rldm_train_pack_weights", ins["w"], N, Cin, 16, out["wf"], out["wt"])
        done(f"pack_weights {(N, Cin, 16)} residue {r}", out, ins)
    same(out["wf"].float(), wf0.float(), f"pack_weights forward copy {(N, Cin, 16)}")
    same(out["wt"].float(), wt0.float(), f"pack_weights transposed copy {(N, Cin, 16)}")
    wv = w.view(N, Cin, 16)
    exact(out["wf"].float()[:, :, :Cin], wv.permute(0, 2, 1), f"pack_weights forward copy {(N, Cin, 16)}", ("n", "tap", "c"))
    exact(out["wt"].float()[:, :, :N], wv.flip(2).permute(1, 2, 0), f"pack_weights transposed copy {(N, Cin, 16)}", ("c", "tap", "n"))


# ---- BatchNorm + LeakyReLU, LeakyReLU ------------------------------------------------------------------------------------------------
BN_SHAPES = [
    (2, 2, 2, 16),
    (3, 5, 7, 32),
    (1, 1, 2, 16),                  # M = 2: the fewest rows the training mode takes
    (3, 10, 10, 80),                # M = 300: two row slices, the second ragged; C = 80: a second channel block of 16
]


@residues
@both_modes
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_lrelu_placed(shape, det, r):
    """Against the same calls on plain allocations, bit for bit in both modes: these kernels have no floating-point atomics, their sums
    are fp64 in a fixed order.  dgamma / dbeta accumulate: the plain call starts them at 0, so it holds (float) s exactly; the placed
    call starts at integers of magnitude <= 100 and the kernel's `+=` is ONE fp32 rounding of pre-fill + (float) s -- which is what the
    host's fp32 addition of the pre-fill and the plain result is, so the two are equal bit for bit."""
    x, gamma, beta, dy, rm, rv = _bn_case(shape)
    Cc, M = shape[-1], int(np.prod(shape[:-1]))
    what = what_of(shape, det, r)
    pre_g, pre_b = int_grid((Cc,), 45, -100, 100), int_grid((Cc,), 46, -100, 100)
    nbytes = _lib.lib().rldm_train_disc_bn_workspace(M, Cc)
    assert nbytes == ((M + 255) // 256) * Cc * 16 + Cc * 8
    with mode(det):
        xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
        rm0, rv0, nbt0 = rm.clone().to(DEV), rv.clone().to(DEV), torch.full((), 6, dtype=torch.int64).to(DEV)
        y0, save0 = D.bn_lrelu_forward(xd, gd, bd, rm0, rv0, nbt0, training=True)
        dg0, db0 = torch.zeros(Cc).to(DEV), torch.zeros(Cc).to(DEV)
        dx0 = D.bn_lrelu_backward(xd, dyd, save0, gd, bd, dg0, db0)
        ye0, se0 = D.bn_lrelu_forward(xd, gd, bd, rm.to(DEV), rv.to(DEV), None, training=False)
        act, par = p_in(x=x, dy=dy), p_in(r, gamma=gamma, beta=beta)
        # forward, training mode
        run = p_acc(r, running_mean=rm, running_var=rv)
        out = p_out(save=(2 * Cc,), y=shape)
        ws, wsp, nb = ws_bytes(nbytes)
        nbt = torch.full((), 6, dtype=torch.int64).to(DEV)
        call("rldm_train_disc_bn_forward", act["x"], M, Cc, par["gamma"], par["beta"], run["running_mean"], run["running_var"], nbt, 1,
             out["save"], out["y"], wsp, nb)
        done("bn_forward " + what, out, run, ws, act, par)
        same(out["y"], y0, "bn_forward y " + what)
        same(out["save"], save0, "bn_forward save " + what)
        same(run["running_mean"], rm0, "bn_forward running_mean " + what)
        same(run["running_var"], rv0, "bn_forward running_var " + what)
        assert int(nbt) == int(nbt0) == 7
        # forward, eval mode: the running statistics are inputs, no workspace
        rin = p_in(r, running_mean=rm, running_var=rv)
        out = p_out(save=(2 * Cc,), y=shape)
        call("rldm_train_disc_bn_forward", act["x"], M, Cc, par["gamma"], par["beta"], rin["running_mean"], rin["running_var"], None, 0,
             out["save"], out["y"], None, 0)
        done("bn_forward eval " + what, out, rin, act, par)
        same(out["y"], ye0, "bn_forward eval y " + what)
        same(out["save"], se0, "bn_forward eval save " + what)
        # backward, with and without the parameter gradients
        sv = p_in(save=save0.cpu())
        g, dxo = p_acc(r, dgamma=pre_g, dbeta=pre_b), p_out(dx=shape)
        ws, wsp, nb = ws_bytes(nbytes)
        call("rldm_train_disc_bn_backward", act["x"], act["dy"], sv["save"], M, Cc, par["gamma"], par["beta"], dxo["dx"], g["dgamma"],
             g["dbeta"], wsp, nb)
        done("bn_backward " + what, dxo, g, ws, act, par, sv)
        same(dxo["dx"], dx0, "bn_backward dx " + what)
        same(g["dgamma"], pre_g + dg0.cpu(), "bn_backward dgamma " + what)
        same(g["dbeta"], pre_b + db0.cpu(), "bn_backward dbeta " + what)
        dxo = p_out(dx=shape)
        ws, wsp, nb = ws_bytes(nbytes)
        call("rldm_train_disc_bn_backward", act["x"], act["dy"], sv["save"], M, Cc, par["gamma"], par["beta"], dxo["dx"], None, None, wsp, nb)
        done("bn_backward, dx alone " + what, dxo, ws, act, par, sv)
        same(dxo["dx"], dx0, "bn_backward, dx alone " + what)


@both_modes
def test_lrelu_placed(det):
    """tests/test_discriminator_gpu.py::test_lrelu_kernel's values and its torch expression (280 elements: two blocks, the second
    ragged)."""
    x = torch.tensor([-2.0, -0.0, 0.0, 0.5, 3.0, -1e-30, 1e-30] * 40)
    dy = torch.linspace(-1, 1, x.numel())
    with mode(det):
        ins, out = p_in(x=x, dy=dy), p_out(y=x.shape, dx=x.shape)
        call("rldm_train_disc_lrelu", ins["x"], None, out["y"], x.numel(), 0)
        call("rldm_train_disc_lrelu", ins["x"], ins["dy"], out["dx"], x.numel(), 1)
        done("lrelu", out, ins)
    exact(out["y"], torch.where(x > 0, x, np.float32(0.2) * x), "lrelu", ("e",))
    exact(out["dx"], torch.where(x > 0, dy, dy * np.float32(0.2)), "lrelu backward", ("e",))


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
@both_modes
@pytest.mark.parametrize("n,factor", [(4, 1.0), (24, 1.0), (1000, 0.75)])
def test_hinge_and_generator_placed(n, factor, det):
    """tests/test_discriminator_gpu.py::test_hinge_and_generator_match_their_numpy_statements' logits, statements and rules: the
    gradients equal hinge_host's; the sums are exact over a power of two and otherwise within its 1e-14 (each term rounded once in
    fp64, then summed).  `partials` holds exactly 3 (1) x ceil(n / 256) doubles; the default mode never writes it."""
    real, fake = _logits(n, 51), _logits(n, 52)
    out_h, dreal_h, dfake_h = D.hinge_host(real.numpy(), fake.numpy(), factor)
    nparts = (n + 255) // 256
    with mode(det):
        ins = p_in(real=real, fake=fake)
        out, words, part = p_out(dreal=(n,), dfake=(n,)), p_out(dtype=F64, out=(3,)), p_ws(F64, partials=3 * nparts)
        call("rldm_train_disc_hinge", ins["real"], ins["fake"], n, factor, out["dreal"], out["dfake"], words["out"], part["partials"])
        done(f"hinge {n}", out, words, part, ins)
        gout, gword, gpart = p_out(dfake=(n,)), p_out(dtype=F64, out=(1,)), p_ws(F64, partials=nparts)
        call("rldm_train_disc_generator", ins["fake"], n, gout["dfake"], gword["out"], gpart["partials"])
        done(f"generator {n}", gout, gword, gpart, ins)
    got, g = words["out"].cpu().numpy(), float(gword["out"][0])
    assert np.array_equal(out["dreal"].cpu().numpy(), dreal_h) and np.array_equal(out["dfake"].cpu().numpy(), dfake_h)
    assert np.array_equal(gout["dfake"].cpu().numpy(), np.full(n, np.float32(-1.0 / n)))
    g_h = -fake.double().numpy().sum() / n
    if n & (n - 1) == 0:
        assert np.array_equal(got, out_h) and g == g_h
    else:
        assert np.allclose(got, out_h, rtol=1e-14, atol=1e-15) and abs(g - g_h) <= 1e-14 * abs(g_h) + 1e-15


@both_modes
def test_adaptive_mix_placed(det):
    """tests/test_discriminator_gpu.py::test_adaptive_mix's operands and numpy expression; the two fp64 squared norms and d_weight are
    placed fp64 views of one element."""
    gen = torch.Generator().manual_seed(61)
    dnll, dg = torch.randn(2, 5, 7, 2, generator=gen), torch.randn(2, 5, 7, 2, generator=gen)
    with mode(det):
        for sq_n, sq_g, dw_, df in ((4.0, 9.0, 0.5, 1.0), (2.5, 1e-12, 0.5, 1.0), (0.0, 3.0, 0.5, 0.25), (7.0, 0.3, 0.8, 1.0)):
            ins = p_in(dnll=dnll, dg=dg)
            sq = p_in(sq_nll=torch.tensor([sq_n], dtype=F64), sq_g=torch.tensor([sq_g], dtype=F64))
            out, w = p_out(dpred=dnll.shape), p_out(dtype=F64, d_weight=(1,))
            call("rldm_train_disc_adaptive_mix", ins["dnll"], ins["dg"], sq["sq_nll"], sq["sq_g"], dw_, df, out["dpred"], w["d_weight"],
                 dnll.numel())
            done(f"adaptive_mix {(sq_n, sq_g, dw_, df)}", out, w, ins, sq)
            got = float(w["d_weight"][0])
            w_h = min(max(np.sqrt(sq_n) / (np.sqrt(sq_g) + 1e-4), 0.0), 1e4) * float(np.float32(dw_))
            assert abs(got - w_h) <= 1e-15 * w_h
            s = np.float32(got * float(np.float32(df)))
            assert np.array_equal(out["dpred"].cpu().numpy(), dnll.numpy() + (s * dg.numpy()).astype(np.float32))


# ---- rldm_train_colsum as the discriminators call it: rows = nullptr, `total` alone -----------------------------------------------------
@residues
@both_modes
@pytest.mark.parametrize("B,npix,N", [(1, 12, 1), (2, 3 * 16, 2), (2, 150 * 16, 16)], ids=lambda v: str(v))
def test_colsum_total_placed(B, npix, N, det, r):
    """(1, 12, 1): the PatchGAN's last bias; (2, 48, 2): db1 / db2 of the C = 2 Meta-Kernel layer, the sum over rows; (2, 2400, 16): an
    MLP bias of a wider layer, ten 256-row slabs per image and 16-byte loads of dy."""
    dy, pre = int_grid((B, npix, N), 811), int_grid((N,), 812, -100, 100)
    assert_exact_bound(1.0, (B * npix, amax(dy)), (1, amax(pre)))
    with mode(det):
        ins, g = p_in(dy=dy), p_acc(r, total=pre)
        call("rldm_train_colsum", ins["dy"], B, npix, N, None, 0, 0, g["total"])
        done(f"colsum {(B, npix, N)} det={det} residue {r}", g, ins)
    exact(g["total"], pre.double() + dy.double().sum((0, 1)), f"colsum total {(B, npix, N)} det={det} residue {r}", ("n",))


# ---- the Meta-Kernel layer -----------------------------------------------------------------------------------------------------------
META_PLACED = [
    (2, 8, 6, 2, 16, 2),            # C = 2: the whole MLP on the fp32 GEMM; the layer whose parameters sit at both residues
    (2, 4, 3, 16, 1, 1),            # N = 1, odd H
    (2, 16, 6, 16, 80, 1),          # several M tiles, N in two tiles, eight K chunks
    (1, 7, 5, 16, 16, 2),           # odd extents at stride 2
]
assert all(c in LAYER_CASES for c in META_PLACED)
GRAD_KEYS = ("dw1", "db1", "dw2", "db2", "dcoov", "dbias")
PARAM_OF = dict(dw1="w1", db1="b1", dw2="w2", db2="b2", dcoov="coov", dbias="bias")


def _prefills(c, ref):
    """Integer pre-fills (|.| <= 100) of the six gradients, and pre-fill + the fp64 reference.  dw1 / dw2 / dcoov: the GEMM (or its
    slice reduction, from 0) forms the whole sum, which exact_layer_case shows to be exact, and adds it to the pre-fill once -- exact
    when the result is an fp32 number, asserted here.  db1 / db2 / dbias: colsum adds into the pre-filled `total` in any order;
    their terms are integers whose absolute sum exact_layer_case keeps below 2^22, so every partial sum on top of the pre-fill is
    an integer below 2^24."""
    pre = {k: int_grid(tuple(c[PARAM_OF[k]].shape), 820 + i, -100, 100) for i, k in enumerate(GRAD_KEYS)}
    want = {k: pre[k].double() + tn(ref[k]).double().reshape(pre[k].shape) for k in GRAD_KEYS}
    for k, v in want.items():
        assert torch.equal(v.float().double(), v), f"{k}: pre-fill + reference is no fp32 number"
        if k in ("db1", "db2", "dbias"):
            assert torch.equal(v, v.round()) and float(v.abs().max()) + 100 < 2 ** 22, k
    return pre, want


@residues
@both_modes
@pytest.mark.parametrize("case", META_PLACED, ids=lambda c: "x".join(map(str, c)))
def test_meta_layer_placed(case, det, r):
    """tests/meta_util.exact_layer_case's operands and fp64 `ref`, as tests/test_metakernel_gpu.py::test_layer_exact asks of the plain
    call: everything EQUAL.  The backward takes the forward's own pe / m (which equal the reference) and src."""
    B, W, H, Cc, N, stride = case
    c = exact_layer_case(*case)
    ref = c["ref"]
    what = what_of(case, det, r)
    d = MK.layer_desc((B, W, H, Cc), N, stride)
    Wo, Ho = D.conv_out_size(W, H, stride)
    rows = B * Wo * Ho * 16
    nbytes = _lib.lib().rldm_train_meta_workspace(C.byref(d))
    assert nbytes >= (2 * rows * Cc + 3 * rows) * 4
    with mode(det):
        act = p_in(x=c["x"], rng=c["r"], tables=c["tables"], dy=c["dy"], dr_next=c["dr_next"])
        par = p_in(r, w1=c["w1"], b1=c["b1"], w2=c["w2"], b2=c["b2"], coov=c["coov"], bias=c["bias"])
        ins = (act, par)
        out = p_out(y=(B, Wo, Ho, N), r_next=(B, Wo, Ho), pe=(rows, 3), m=(rows, Cc))
        src = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        ws, wsp, nb = ws_bytes(nbytes)
        call("rldm_train_meta_forward", C.byref(d), act["x"], act["rng"], act["tables"], par["w1"], par["b1"], par["w2"], par["b2"],
             par["coov"], par["bias"], out["y"], out["r_next"], out["pe"], src, out["m"], wsp, nb)
        done("meta_forward " + what, out, ws, *ins)
        exact(out["pe"], tn(ref["pe"]), "pe " + what, ("row", "e"))
        assert torch.equal(src.cpu(), tn(ref["src"])), "src " + what
        exact(out["m"], tn(ref["m"]), "m " + what, ("row", "c"))
        exact(out["y"], tn(ref["y"]), "output " + what, ("image", "w", "h", "n"))
        exact(out["r_next"], tn(ref["r_next"]), "returned r " + what, ("image", "w", "h"))
        sv = p_in(pe=out["pe"].cpu(), m=out["m"].cpu())
        pre, want = _prefills(c, ref)

        def backward(params, want_input):
            g = p_acc(r, **pre) if params else None
            go = p_out(dx=(B, W, H, Cc), dr=(B, W, H)) if want_input else None
            ws, wsp, nb = ws_bytes(nbytes)
            gp = [g[k] for k in GRAD_KEYS] if params else [None] * 6
            call("rldm_train_meta_backward", C.byref(d), act["x"], act["dy"], act["tables"], par["w1"], par["b1"], par["w2"], par["coov"],
                 sv["pe"], src, sv["m"], act["dr_next"] if want_input else None, go["dx"] if want_input else None,
                 go["dr"] if want_input else None, *gp, wsp, nb)
            w2_ = f"meta_backward params={params} input={want_input} " + what
            done(w2_, ws, sv, *ins, *([g] if params else []), *([go] if want_input else []))
            if want_input:
                exact(go["dx"], tn(ref["dx"]), "dx " + w2_, ("image", "w", "h", "c"))
                exact(go["dr"], tn(ref["dr"]), "dr " + w2_, ("image", "w", "h"))
            if params:
                for k in GRAD_KEYS:
                    exact(g[k], want[k], f"{k} {w2_}", ("n", "k")[:g[k].dim()])
        backward(True, True)
        backward(False, True)                                   # the input gradient alone
        backward(True, False)                                   # the parameters alone
        assert torch.equal(src.cpu(), tn(ref["src"])), "src was modified " + what


@both_modes
@pytest.mark.parametrize("case", [META_PLACED[0], META_PLACED[3]], ids=lambda c: "x".join(map(str, c)))
def test_meta_range_placed(case, det):
    """r = (x[..., 0] 40 + 20) / 10 on x in {-1, 0, 1}: {-2, 2, 6}; dx[..., 0] += (dr / 10) 40 on dr in 10 {-3 .. 3}: exact."""
    B, W, H, Cc, N, stride = case
    x = exact_layer_case(*case)["x"]
    dr, pre = 10 * int_grid((B, W, H), 831), int_grid((B, W, H, Cc), 832, -100, 100)
    with mode(det):
        ins, out = p_in(x=x), p_out(rng=(B, W, H))
        call("rldm_train_meta_range", ins["x"], B * W * H, Cc, 20.0, 40.0, out["rng"])
        done(f"meta_range {case}", out, ins)
        exact(out["rng"], (x[..., 0].double() * 40 + 20) / 10, f"meta_range {case}", ("image", "w", "h"))
        din, acc = p_in(dr=dr), p_acc(dx=pre)
        call("rldm_train_meta_range_grad", din["dr"], B * W * H, Cc, 40.0, acc["dx"])
        done(f"meta_range_grad {case}", acc, din)
        want = pre.double().clone()
        want[..., 0] += dr.double() / 10 * 40
        exact(acc["dx"], want, f"meta_range_grad {case}", ("image", "w", "h", "c"))


# ---- BEV: to_voxel_train / to_voxel_backward ------------------------------------------------------------------------------------------
BEV_GRID, BEV_RANGE = min(BU.SPLAT_GRIDS, key=lambda g: int(np.prod(g[0])))


@pytest.mark.parametrize("channels", [2, 3], ids=["C2", "C3-nan-channel"])
@pytest.mark.parametrize("bev_mode", BU.MODES)
def test_to_voxel_train_and_backward_placed(bev_mode, channels):
    """tests/bev_util.py's smallest grid and input: image 0 dense with re-encoded negative ranges (replaced by the fill), image 1 all
    but empty (points outside the volume: dropped).  C = 3: a third channel of NaN that no kernel may read.

    Forward (fp32 atomics): the placed call's raw accumulators and output planes within the per-cell bounds
    test_forward_keeps_the_accumulators_and_to_voxels_bounds states against the fp64 accumulation of the device's own votes
    (BU.splat_reference / BU.splat_bounds; E_n as there), and against the plain-allocation call: both are fp32 sums of the same k votes
    in some order, each within E_d (E_n) of the exact sum, so they differ by at most 2 E_d (2 E_n) -- 0 for a cell with one vote.  Cells
    no pixel reaches are exactly 0 in all four planes.
    Backward (a gather, no atomics): the placed and the plain call get the same raw and must agree bit for bit; dropped pixels are
    exactly 0 in both channels -- and written, which done() checks."""
    U = BU.U
    img2 = np.array(BU.bev_input(BEV_GRID, BEV_RANGE, bev_mode)[0])
    B, _, W, H = img2.shape
    img = img2 if channels == 2 else np.concatenate([img2, np.full((B, 1, W, H), np.nan, BU.F)], 1)
    gz, gy, gx = BEV_GRID
    vshape = (B, 2 * gz, gy, gx)
    G = BU.upstream(vshape)
    for normalize in (False, True):
        t = BU.bev_sensor(BEV_GRID, BEV_RANGE, bev_mode, normalize)
        o = BU.oracle_of(t)
        what = f"{bev_mode} C={channels} normalize={normalize}"
        x2 = torch.from_numpy(img2).to(DEV)
        pts = t.to_pc_torch(x2).cpu()
        vox0, (_, raw0) = t.to_voxel_train(x2)
        ins = p_in(img=torch.from_numpy(img))
        out = p_out(raw=vshape, voxel=vshape)
        call("rldm_lidar_to_voxel_train", t._handle(), ins["img"], B, channels, W, out["raw"], out["voxel"])
        done("to_voxel_train " + what, out, ins)
        raw, vox = out["raw"].cpu().numpy().astype(np.float64), out["voxel"].cpu().numpy().astype(np.float64)
        plain_raw, plain_vox = raw0.cpu().numpy().astype(np.float64), vox0.cpu().numpy().astype(np.float64)
        ref = BU.splat_reference(o, pts.numpy())
        e_d, bound_d, bound_f = BU.splat_bounds(ref)
        occ = ref["k"] > 0
        km1 = np.maximum(ref["k"] - 1, 0)
        gamma = km1 * U / (1 - km1 * U)
        e_n = U * ref["swf_abs"] + gamma * (1 + U) * ref["swf_abs"]
        assert occ.any() and (~occ).any()
        assert np.array_equal(raw[:, :gz] != 0, occ) and (raw[:, gz:][~occ] == 0).all() and (vox[~np.concatenate([occ, occ], 1)] == 0).all()
        assert (np.abs(raw[:, :gz] - ref["sw"]) <= bound_d).all() and (np.abs(raw[:, gz:] - ref["swf"]) <= e_n + U * np.abs(ref["swf"])).all()
        want = o.to_voxel(img2, pc=pts.numpy()).astype(np.float64)
        assert np.isfinite(vox).all()
        assert (np.abs(vox[:, :gz] - want[:, :gz]) <= bound_d + (2e-5 if normalize else 0.0)).all()
        assert (np.abs(vox[:, gz:] - want[:, gz:]) <= bound_f).all()
        # ... and against the plain-allocation call
        assert (np.abs(raw[:, :gz] - plain_raw[:, :gz]) <= 2 * e_d).all() and (np.abs(raw[:, gz:] - plain_raw[:, gz:]) <= 2 * e_n).all()
        one = ref["k"] <= 1
        assert one.any() and np.array_equal(raw[:, :gz][one], plain_raw[:, :gz][one]) and np.array_equal(vox[:, :gz][one], plain_vox[:, :gz][one])
        if not normalize:
            assert np.array_equal(vox[:, :gz], raw[:, :gz])
        # backward on the plain call's raw
        bins = p_in(img=torch.from_numpy(img), raw=raw0.cpu(), dvoxel=torch.from_numpy(G))
        bout = p_out(cell_grad=vshape, dimages=(B, 2, W, H))
        call("rldm_lidar_to_voxel_backward", t._handle(), bins["img"], B, channels, W, bins["raw"], bins["dvoxel"], bout["cell_grad"],
             bout["dimages"])
        done("to_voxel_backward " + what, bout, bins)
        plain = t.to_voxel_backward((x2, raw0), torch.from_numpy(G).to(DEV))
        same(bout["dimages"], plain, "to_voxel_backward " + what)
        cls = BU.pixel_classes(t, img2, points=pts)
        dropped, replaced = torch.from_numpy(cls["dropped"]), torch.from_numpy(cls["replaced"])
        got = bout["dimages"].cpu()
        assert dropped.sum() >= 40 and (got[:, 0][dropped] == 0).all() and (got[:, 1][dropped] == 0).all()
        assert (got[:, 0][replaced] == 0).all() and (bev_mode == "inverse" or replaced.sum() >= 20)
        assert (got[:, 0][~dropped & ~replaced] != 0).float().mean() > 0.9
