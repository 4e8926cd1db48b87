"""GPU: the PatchGAN discriminator (rangeldm_amd/discriminator.py, csrc/train_disc.hip) and the VAE trainers' adversarial phase.

Exact: the 4x4 zero-padded convs (forward, data gradient, weight gradient, bias sum) on integer grids against fp64
F.conv2d(padding=1) autograd, bit for bit in both modes of the library; the W boundary (no wrap); the refusals; LeakyReLU; the hinge /
generator sums on dyadic logits; the gradient mix.

Counted: BatchNorm + LeakyReLU against discriminator.batchnorm_host (fp64).  BN_FWD / BN_BWD are the numbers of fp32 roundings of the
kernel's expressions, each at most 2^-24 relative to the terms it rounds:
    y  = lrelu(((x - mean) rstd) gamma + beta)         mean -> fp32, x - mean, rstd -> fp32, * rstd, * gamma, + beta, * 0.2        7 -> 8
    dx = (gamma rstd) ((dz - k1) - xhat k2)            dz = dy * slope, k1 -> fp32, k2 -> fp32, xhat (4), xhat * k2, dz - k1,
                                                       (...) - (...), gamma * rstd (rstd's rounding counted again), the product      13 -> 16
against terms_y = (|x| + |mean|) rstd |gamma| + |beta| and terms_dx = |gamma| rstd (|dz| + |k1| + (|x| + |mean|) rstd |k2|).  An element
whose fp64 z is closer to 0 than its own rounding bound (and is not an exact 0) may take the other LeakyReLU branch in fp32; such
elements are counted and left out (none at these seeds but the count is asserted small).

Measured (test_network_matches_the_golden, test_adversarial_*): the project's rule from tests/test_vae_training_gpu.py -- relative L2
per parameter (with the floor of tests/test_training.py) and over the flat buffer, worst of three runs on an MI355X, gated at twice
that rounded up to two digits -- printed next to the distance of forward_host(bf16=True) from the same golden, computed on the host.
GATES / STEP_GATES hold the gates; the measured figures stand beside them."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rangeldm_amd import discriminator as D
from tests.disc_util import PATCH as U
from tests.disc_util import mode, nchw, nhwc
from tests.disc_util import param_errors as _param_errors
from tests.hip_util import amax, assert_bitexact, assert_exact_bound, int_grid

pytestmark = pytest.mark.gpu
UNIT = 2.0 ** -5


# ---- the 4x4 convs, exact --------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # (B, Cin, N, W, H, stride)
    (1, 2, 64, 8, 64, 2),           # the first layer's beams
    (2, 64, 128, 4, 32, 2),
    (1, 128, 256, 4, 16, 2),
    (1, 256, 512, 4, 8, 1),         # output 3 x 7
    (1, 512, 1, 3, 7, 1),           # output 2 x 6, N = 1
    (1, 16, 16, 2, 2, 2),           # one output pixel, most taps in the padding
    (1, 16, 16, 2, 2, 1),
    (3, 32, 48, 7, 5, 2),           # odd batch, odd extents 7 -> 3 and 5 -> 2
    (1, 16, 16, 4, 2, 2),           # Hout = 1
]
_CONV_REF = {}


def _conv_reference(case):
    if case not in _CONV_REF:
        B, Cin, N, W, H, stride = case
        x = int_grid((B, Cin, W, H), 701)
        w = int_grid((N, Cin, 4, 4), 702, -4, 4, exp=-5)
        bias = int_grid((N,), 703, -64, 64, exp=-5)
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        ref = F.conv2d(x64, w64, bias.double(), stride=stride, padding=1)
        assert tuple(ref.shape[2:]) == D.conv_out_size(W, H, stride)
        dy = int_grid(ref.shape, 705)
        ref.backward(dy.double())
        P = B * ref.shape[2] * ref.shape[3]
        assert_exact_bound(UNIT, (Cin * 16, amax(x) * amax(w)), (1, amax(bias)))
        assert_exact_bound(UNIT, (N * 16, amax(dy) * amax(w)))
        assert_exact_bound(1.0, (P, amax(dy) * amax(x)))
        _CONV_REF[case] = (x, w, bias, dy, ref.detach(), x64.grad, w64.grad)
    return _CONV_REF[case]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv4_exact(case, det):
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H, stride = case
    x, w, bias, dy, ref, dx_ref, dw_ref = _conv_reference(case)
    what = f"{case} {'deterministic' if det else 'default'}"
    with mode(det):
        wf, wt = T.pack_weights(w.cuda(), 16)
        xd, dyd = nhwc(x), nhwc(dy)
        y = D.conv4(xd, wf, N, stride, bias.cuda())
        assert_bitexact(nchw(y), ref.float(), what="conv " + what)
        y0 = D.conv4(xd, wf, N, stride)
        assert_bitexact(nchw(y0), (ref - bias.double()[None, :, None, None]).float(), what="conv without bias " + what)
        dx = D.conv4_dgrad(dyd, wt, xd.shape, stride)
        assert_bitexact(nchw(dx), dx_ref.float(), what="data gradient " + what)
        dw, db = torch.zeros_like(w).cuda(), torch.zeros(N).cuda()
        D.conv4_wgrad(dyd, xd, dw, stride, db)
        assert_bitexact(dw.cpu(), dw_ref.float(), names=("n", "cin", "i", "j"), what="weight gradient " + what)
        assert_bitexact(db.cpu(), dy.sum((0, 2, 3)), names=("n",), what="bias sum " + what)
        D.conv4_wgrad(dyd, xd, dw, stride)                       # (added into what dw holds, as rldm_train_wgrad)
        assert_bitexact(dw.cpu(), 2 * dw_ref.float(), names=("n", "cin", "i", "j"), what="weight gradient, second call " + what)


def test_conv4_weight_gradient_with_many_slices():
    """More output pixels than one K slice holds (several slices, the reduction in slice order), at the first layer's channel counts and
    at a 64-channel pair: the sliced path of rldm_train_disc_wgrad, exact."""
    for B, Cin, N, W, H, stride in ((2, 2, 64, 64, 32, 2), (1, 64, 64, 64, 16, 2)):
        x, dy = int_grid((B, Cin, W, H), 711), int_grid((B, N, W // 2, H // 2), 712)
        x64 = x.double()
        w64 = torch.zeros(N, Cin, 4, 4, dtype=torch.float64, requires_grad=True)
        F.conv2d(x64, w64, None, stride=stride, padding=1).backward(dy.double())
        assert_exact_bound(1.0, (B * (W // 2) * (H // 2), amax(dy) * amax(x)))
        d = D.conv_desc((B, W, H, Cin), N, stride)
        assert D._lib.lib().rldm_train_disc_wgrad_workspace(d) > 0
        dw = torch.zeros(N, Cin, 4, 4).cuda()
        D.conv4_wgrad(nhwc(dy), nhwc(x), dw, stride)
        assert_bitexact(dw.cpu(), w64.grad.float(), names=("n", "cin", "i", "j"), what=f"sliced weight gradient {(B, Cin, N, W, H)}")


@pytest.mark.parametrize("stride", [1, 2])
def test_conv4_does_not_wrap_w(stride):
    """Nonzero values in column W - 1 alone: output column 0 reads column -1 under tap i = 0, which is padding here (zero) and would be
    column W - 1 in a conv that wraps W -- the reference differs between the two, and the kernel gives the zero-padded one."""
    from rangeldm_amd import train_ops as T
    B, Cin, N, W, H = 1, 16, 16, 8, 6
    x = torch.zeros(B, Cin, W, H)
    x[:, :, W - 1] = int_grid((B, Cin, H), 721, 1, 3)
    w = int_grid((N, Cin, 4, 4), 722, 1, 4, exp=-5)
    ref = F.conv2d(x.double(), w.double(), None, stride=stride, padding=1)
    wrapped = F.conv2d(F.pad(F.pad(x.double(), (0, 0, 1, 1), mode="circular"), (1, 1, 0, 0)), w.double(), None, stride=stride)
    assert wrapped.shape == ref.shape and float(ref[:, :, 0].abs().max()) == 0.0 and float(wrapped[:, :, 0].abs().min()) > 0.0
    wf, wt = T.pack_weights(w.cuda(), 16)
    y = nchw(D.conv4(nhwc(x), wf, N, stride))
    assert_bitexact(y, ref.float(), what="W boundary")
    assert float(y[:, :, 0].abs().max()) == 0.0
    # and the data gradient: dy in output column 0 alone must not reach input column W - 1
    dy = torch.zeros_like(ref, dtype=torch.float32)
    dy[:, :, 0] = int_grid(dy[:, :, 0].shape, 723, 1, 3)
    dx = nchw(D.conv4_dgrad(nhwc(dy), wt, (B, W, H, Cin), stride))
    assert float(dx[:, :, W - 1].abs().max()) == 0.0 and float(dx[:, :, 0].abs().max()) > 0.0


def test_shapes_without_an_instance_are_refused():
    from rangeldm_amd import train_ops as T
    for shape, N, stride in (((1, 8, 8, 3), 16, 2), ((1, 8, 8, 24), 16, 1), ((1, 8, 8, 16), 8, 2), ((1, 8, 8, 16), 16, 3),
                             ((1, 1, 8, 16), 16, 1), ((1, 8, 1, 16), 16, 2), ((1, 8, 8, 16), 0, 1)):
        with pytest.raises(ValueError, match="no 4x4 discriminator conv instance"):
            D.conv_desc(shape, N, stride)
    x = torch.zeros(1, 8, 8, 24).cuda()
    wf, _ = T.pack_weights(torch.zeros(16, 24, 4, 4).cuda(), 16)
    with pytest.raises(ValueError):
        D.conv4(x, wf, 16, 1)
    import ctypes
    d = D._lib.TrainDiscConvDescC(1, 8, 8, 24, 16, 1)                # the library itself says no, too
    assert ctypes.sizeof(d) == 24
    assert D._lib.lib().rldm_train_disc_conv(ctypes.byref(d), None, None, None, None, None) != 0
    assert b"no instance" in D._lib.lib().rldm_last_error()
    assert D._lib.lib().rldm_train_disc_wgrad_workspace(ctypes.byref(d)) < 0


# ---- BatchNorm + LeakyReLU -----------------------------------------------------------------------------------------------------------
BN_FWD, BN_BWD, E24 = 8, 16, 2.0 ** -24


def _bn_case(shape):
    g = torch.Generator().manual_seed(41 + shape[-1] + shape[0])
    Cc = shape[-1]
    M = int(np.prod(shape[:-1]))
    x = torch.randn(shape, generator=g) * 1.5 + 0.4
    gamma, beta = 1 + 0.3 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    x2 = x.view(M, Cc)
    # channel 0: values symmetric about 0 with exact zeros, beta 0 -> mean == 0 exactly and z == 0 exactly where x == 0: the tie
    half = M // 2
    v = int_grid((half,), 43, 1, 6, exp=-2)
    x2[:half, 0], x2[half:2 * half, 0] = v, -v
    if M % 2:
        x2[-1, 0] = 0.0
    x2[0, 0] = x2[half, 0] = 0.0
    beta[0] = 0.0
    # channel 1: constant zero (variance 0: rstd = 1 / sqrt(eps)), z == beta == 0 everywhere
    x2[:, 1] = 0.0
    beta[1] = 0.0
    dy = torch.randn(shape, generator=g)
    rm, rv = 0.1 * torch.randn(Cc, generator=g), 0.5 + torch.rand(Cc, generator=g)
    return x, gamma, beta, dy, rm, rv


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("shape", [(2, 2, 2, 16), (3, 5, 7, 32), (8, 16, 8, 128), (1, 1, 2, 16)], ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_lrelu_against_its_host_statement(shape, det):
    x, gamma, beta, dy, rm, rv = _bn_case(shape)
    Cc, M = shape[-1], int(np.prod(shape[:-1]))
    h = D.batchnorm_host(x.numpy(), gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy(), True, dy.numpy())
    with mode(det):
        rmd, rvd, nbt = rm.clone().cuda(), rv.clone().cuda(), torch.full((), 6, dtype=torch.int64).cuda()
        xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
        y, save = D.bn_lrelu_forward(xd, gd, bd, rmd, rvd, nbt, training=True)
        dgamma, dbeta = torch.zeros(Cc).cuda(), torch.zeros(Cc).cuda()
        dx = D.bn_lrelu_backward(xd, dyd, save, gd, bd, dgamma, dbeta)
        dx_only = D.bn_lrelu_backward(xd, dyd, save, gd, bd)
        y_eval, save_eval = D.bn_lrelu_forward(xd, gd, bd, rm.cuda(), rv.cuda(), None, training=False)
    assert int(nbt) == 7
    x64, mean, rstd, g64, b64 = x.double().numpy(), h["mean"], h["rstd"], gamma.double().numpy(), beta.double().numpy()
    # statistics: fp64 sums rounded once
    save = save.cpu().double().numpy()
    assert np.all(np.abs(save[:Cc] - mean) <= E24 * np.abs(mean) + 1e-300) and np.all(np.abs(save[Cc:] - rstd) <= 2 * E24 * rstd)
    assert np.all(np.abs(rmd.cpu().double().numpy() - h["running_mean"]) <= 2 * E24 * (np.abs(0.9 * rm.numpy()) + np.abs(0.1 * mean)))
    assert np.all(np.abs(rvd.cpu().double().numpy() - h["running_var"]) <= 2 * E24 * h["running_var"])
    # forward
    xh = (x64 - mean) * rstd
    z = xh * g64 + b64
    zbound = BN_FWD * E24 * ((np.abs(x64) + np.abs(mean)) * rstd * np.abs(g64) + np.abs(b64))
    risky = (np.abs(z) <= zbound) & (z != 0)
    assert risky.sum() <= 2, int(risky.sum())
    ey = np.abs(y.cpu().double().numpy() - h["y"])
    assert np.all(ey[~risky] <= zbound[~risky]), float((ey / (zbound + 1e-300))[~risky].max())
    tie = (z == 0)
    assert tie[..., 0].sum() >= 2 and tie[..., 1].all()                # the tie is hit: exact zeros in channels 0 and 1
    assert np.all(y.cpu().numpy()[tie] == 0.0)
    # backward
    dz = dy.double().numpy() * np.where(z > 0, 1.0, 0.2)
    k1, k2 = h["dbeta"] / M, h["dgamma"] / M
    xterms = (np.abs(x64) + np.abs(mean)) * rstd
    tdx = np.abs(g64) * rstd * (np.abs(dz) + np.abs(k1) + xterms * np.abs(k2))
    edx = np.abs(dx.cpu().double().numpy() - h["dx"])
    print(f"bn {shape} det={det}: y {float((ey / (zbound / BN_FWD + 1e-300))[~risky].max()):.2f}, dx "
          f"{float((edx / (tdx * E24 + 1e-300))[~risky].max()):.2f} (units of 2^-24 of the terms)")
    assert np.all(edx[~risky] <= BN_BWD * E24 * tdx[~risky])
    assert torch.equal(dx_only, dx)                                    # the input gradient alone is the same launch without the sums
    # at the tie the gradient is the 0.2 side: where dz's own term dominates, dx moves with 0.2 dy, not with dy
    assert np.all(np.abs(dbeta.cpu().double().numpy() - h["dbeta"]) <= 4 * E24 * np.abs(dz).reshape(-1, Cc).sum(0) + 1e-300)
    assert np.all(np.abs(dgamma.cpu().double().numpy() - h["dgamma"]) <= 8 * E24 * (np.abs(dz) * xterms).reshape(-1, Cc).sum(0) + 1e-300)
    tie_slope = D.batchnorm_host(x.numpy(), gamma.numpy(), beta.numpy(), dy=dy.numpy())["dbeta"][1]
    assert abs(tie_slope - 0.2 * float(dy.double().reshape(-1, Cc)[:, 1].sum())) < 1e-12     # channel 1 is all tie: dbeta = 0.2 sum dy
    assert abs(float(dbeta[1]) - tie_slope) <= 4 * E24 * float(dy.double().reshape(-1, Cc)[:, 1].abs().sum())
    # eval mode: the running statistics, nothing updated
    he = D.batchnorm_host(x.numpy(), gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy(), False)
    ze = BN_FWD * E24 * ((np.abs(x64) + np.abs(he["mean"])) * he["rstd"] * np.abs(g64) + np.abs(b64))
    assert np.all(np.abs(y_eval.cpu().double().numpy() - he["y"]) <= ze)
    assert torch.equal(save_eval[:Cc].cpu(), rm)


def test_batchnorm_needs_two_values_per_channel():
    x = torch.randn(1, 1, 1, 16).cuda()
    one, zero = torch.ones(16).cuda(), torch.zeros(16).cuda()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        D.bn_lrelu_forward(x, one, zero, zero.clone(), one.clone(), torch.zeros((), dtype=torch.int64).cuda(), training=True)
    ws = torch.empty(1024, dtype=torch.uint8).cuda()
    rc = D._lib.lib().rldm_train_disc_bn_forward(D._p(x), 1, 16, D._p(one), D._p(zero), None, None, None, 1, D._p(zero.clone().repeat(2)),
                                                 D._p(torch.empty_like(x)), D._p(ws), 1024, D._s(x))
    assert rc != 0 and b"more than 1 value" in D._lib.lib().rldm_last_error()
    y, _ = D.bn_lrelu_forward(x, one, zero, zero.clone(), one.clone(), None, training=False)          # eval mode takes one value
    assert torch.isfinite(y).all()


def test_lrelu_kernel():
    x = torch.tensor([-2.0, -0.0, 0.0, 0.5, 3.0, -1e-30, 1e-30] * 40).cuda()
    dy = torch.linspace(-1, 1, x.numel()).cuda()
    y, dx = D.lrelu(x), D.lrelu_backward(x, dy)
    assert torch.equal(y.cpu(), torch.where(x.cpu() > 0, x.cpu(), np.float32(0.2) * x.cpu()))
    assert torch.equal(dx.cpu(), torch.where(x.cpu() > 0, dy.cpu(), dy.cpu() * np.float32(0.2)))
    xc = x.cpu().clone().requires_grad_()
    F.leaky_relu(xc, 0.2).backward(dy.cpu())
    assert torch.equal(dx.cpu(), xc.grad)                            # torch's side of the tie at +-0: the slope 0.2


# ---- losses -----------------------------------------------------------------------------------------------------------------------------
def _logits(n, seed):
    """Dyadic logits (multiples of 1/8 in [-4, 4]) with the hinges' corners +-1 among them: every sum below is exact in fp64 in any
    order when n is a power of two."""
    v = int_grid((n,), seed, -32, 32, exp=-3)
    v[:4] = torch.tensor([1.0, -1.0, 1.125, -0.875])[:min(4, n)]
    return v


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("n,factor", [(4, 1.0), (512, 1.0), (1024, 0.5), (24, 1.0), (1000, 0.75)])
def test_hinge_and_generator_match_their_numpy_statements(n, factor, det):
    real, fake = _logits(n, 51), _logits(n, 52)
    out_h, dreal_h, dfake_h = D.hinge_host(real.numpy(), fake.numpy(), factor)
    with mode(det):
        out, dreal, dfake = D.hinge(real.cuda(), fake.cuda(), factor)
        g, dg = D.generator_loss(fake.cuda())
    out, g = out.cpu().numpy(), float(g)
    assert np.array_equal(dreal.cpu().numpy(), dreal_h) and np.array_equal(dfake.cpu().numpy(), dfake_h)
    assert dreal_h[0] == 0 and dreal_h[1] != 0 and dfake_h[1] == 0 and dfake_h[0] != 0          # relu's corner: gradient 0 at 1 -+ logit == 0
    assert np.array_equal(dg.cpu().numpy(), np.full(n, np.float32(-1.0 / n)))
    g_h = -fake.double().numpy().sum() / n
    if n & (n - 1) == 0:                                             # dyadic terms over a power of two: exact, any order, both modes
        assert np.array_equal(out, out_h) and g == g_h
    else:                                                            # each term rounded once in fp64, then summed
        assert np.allclose(out, out_h, rtol=1e-14, atol=1e-15) and abs(g - g_h) <= 1e-14 * abs(g_h) + 1e-15
    ref = D.hinge_d_loss_host(real, fake, factor)
    assert abs(out[0] - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))


def test_adaptive_mix():
    g = torch.Generator().manual_seed(61)
    dnll, dg = torch.randn(2, 5, 7, 2, generator=g), torch.randn(2, 5, 7, 2, generator=g)
    for sq_n, sq_g, dw_, df in ((4.0, 9.0, 0.5, 1.0), (2.5, 1e-12, 0.5, 1.0), (0.0, 3.0, 0.5, 0.25), (7.0, 0.3, 0.8, 1.0)):
        a, b = torch.tensor(sq_n, dtype=torch.float64).cuda(), torch.tensor(sq_g, dtype=torch.float64).cuda()
        dpred, w = D.adaptive_mix(dnll.cuda(), dg.cuda(), a, b, dw_, df)
        w_h = min(max(np.sqrt(sq_n) / (np.sqrt(sq_g) + 1e-4), 0.0), 1e4) * float(np.float32(dw_))
        assert abs(float(w) - w_h) <= 1e-15 * w_h
        s = np.float32(float(w) * float(np.float32(df)))
        assert np.array_equal(dpred.cpu().numpy(), dnll.numpy() + (s * dg.numpy()).astype(np.float32))
        ref = D.adaptive_weight_host(torch.tensor([np.sqrt(sq_n)]), torch.tensor([np.sqrt(sq_g)]), dw_)
        assert abs(float(w) - float(ref)) <= 1e-6 * max(float(ref), 1e-30)
    assert float(D.adaptive_mix(dnll.cuda(), dg.cuda(), a, torch.zeros((), dtype=torch.float64).cuda(), 0.5, 1.0)[1]) == 0.5 * 1e4


# ---- the network against the golden ------------------------------------------------------------------------------------------------------
def _dx_figures(tag, got, ref):
    """The input gradients as whole tensors."""
    return {tag + "_dx": max(U.rel(got[k], ref[k]) for k in ("real", "fake") if k in ref)}


def network_figures(ndf, W, H, det=False):
    """One run of the golden's sequence on the device -> the figures the gates are about (and the same for forward_host(bf16=True))."""
    return U.network_figures(ndf, W, H, _dx_figures, det)


GATE_KEYS = ("logits", "d_loss", "g_loss", "d_worst", "d_all", "d_dx", "g_worst", "g_all", "g_dx", "running")
# worst of three runs on an MI355X -> gate = twice that, rounded up to two digits (the host's bf16 floor beside it in the printout)
# measured: the device's worst of three (forward_host(bf16=True)'s distance from the same golden).  The two agree to two digits
# everywhere: what stands here is the bf16 rounding of the conv operands, amplified by BatchNorm over 12 to 256 values per channel and
# by the hinge's active set -- not the kernels.
GATES = {
    # measured logits 0.00717 (0.00717), d_loss 0.000981 (0.000981), g_loss 0.00578 (0.00578), d_worst 0.119 (0.119), d_all 0.0869 (0.0869),
    # d_dx 0.116 (0.116), g_worst 0.0721 (0.0721), g_all 0.0459 (0.0459), g_dx 0.0653 (0.0653), running 0.00281 (0.00281)
    (16, 32, 24): dict(logits=0.015, d_loss=0.002, g_loss=0.012, d_worst=0.24, d_all=0.18, d_dx=0.24, g_worst=0.15, g_all=0.092, g_dx=0.14,
                       running=0.0057),
    # measured logits 0.0203 (0.0213), d_loss 0.001 (0.000932), g_loss 0.0072 (0.00829), d_worst 0.111 (0.11), d_all 0.0719 (0.0719),
    # d_dx 0.0921 (0.0922), g_worst 0.107 (0.107), g_all 0.0697 (0.0697), g_dx 0.0921 (0.0922), running 0.00288 (0.00288)
    (64, 32, 24): dict(logits=0.041, d_loss=0.0021, g_loss=0.015, d_worst=0.23, d_all=0.15, d_dx=0.19, g_worst=0.22, g_all=0.14, g_dx=0.19,
                       running=0.0058),
    # measured logits 0.00741 (0.00732), d_loss 0.000379 (0.000403), g_loss 0.00759 (0.00818), d_worst 0.134 (0.131), d_all 0.0844 (0.082),
    # d_dx 0.114 (0.111), g_worst 0.118 (0.113), g_all 0.0656 (0.0632), g_dx 0.11 (0.107), running 0.00219 (0.00218)
    (16, 64, 32): dict(logits=0.015, d_loss=0.00076, g_loss=0.016, d_worst=0.27, d_all=0.17, d_dx=0.23, g_worst=0.24, g_all=0.14, g_dx=0.22,
                       running=0.0044),
    # measured logits 0.00763 (0.00781), d_loss 0.000225 (8.24e-05), g_loss 0.00209 (0.00226), d_worst 0.113 (0.114), d_all 0.0788 (0.0777),
    # d_dx 0.0952 (0.0927), g_worst 0.0911 (0.0877), g_all 0.0519 (0.0499), g_dx 0.0931 (0.0893), running 0.00214 (0.00214)
    (64, 64, 32): dict(logits=0.016, d_loss=0.00045, g_loss=0.0042, d_worst=0.23, d_all=0.16, d_dx=0.2, g_worst=0.19, g_all=0.11, g_dx=0.19,
                       running=0.0043),
}


@pytest.mark.parametrize("ndf,W,H", U.CASES)
def test_network_matches_the_golden(ndf, W, H):
    fig, floor = network_figures(ndf, W, H)
    print(f"ndf {ndf} {W}x{H}: " + ", ".join(f"{k} {fig[k]:.3g} (bf16 floor {floor[k]:.3g})" for k in GATE_KEYS)
          + f"; worst d {fig['d_worst_name']}, worst g {fig['g_worst_name']}")
    gates = GATES[(ndf, W, H)]
    bad = {k: (fig[k], gates[k]) for k in GATE_KEYS if not fig[k] <= gates[k]}
    assert not bad, bad


def test_discriminator_step_is_bit_reproducible_in_deterministic_mode():
    U.check_step_is_bit_reproducible()


def test_discriminator_state_round_trip(tmp_path):
    U.check_state_round_trip(tmp_path)


# ---- the adversarial phase of the VAE trainers ------------------------------------------------------------------------------------------
# The VAE config is tests/test_vae_training_gpu.py's SMALL (32 x 8 images).  8 beams leave no room for three stride-2 layers (8 -> 4 -> 2
# -> 1 -> 0), so the discriminator of these tests is the same network with n_layers = 1 (main.0 stride 2, main.2 + BatchNorm stride 1,
# main.5): 32 x 8 -> 16 x 4 -> 15 x 3 -> 14 x 2 logits.  The stride-2 BatchNorm layers are covered by the golden cases above.
WC = (40.0, 10.0)
DCFG = D.DiscriminatorConfig(2, 16, 1)
_ADV = {}


def adv_case():
    """Once: SMALL's weights, a latent batch, an L1 target with a sign margin, the discriminator's state, and the host reference of one
    adversarial step of VAEDecoderTrainer: autograd of nll + d_weight g_loss (d_weight detached) on the oracle decoder + forward_host,
    and torch Adam on the discriminator for hinge(real = target, fake = the oracle's prediction)."""
    if not _ADV:
        from oracle import vae as o_vae
        from rangeldm_amd.params import vae_param_shapes
        from rangeldm_amd.synth import synth_state_dict
        from tests.test_vae_training_gpu import SMALL
        cfg, B, lr = SMALL, 3, 1e-3
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(7)
        f = cfg.downscale
        z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        keys = [k for k in sd if k.startswith("decoder.")]
        sdt = {k: torch.from_numpy(np.array(sd[k])).float().requires_grad_() for k in keys}
        pred = o_vae.vae_decode.__wrapped__(sdt, cfg, z)
        s = torch.randint(0, 2, pred.shape, generator=g).float() * 2 - 1
        target = (pred.detach() + s * (0.25 + 0.25 * torch.rand(pred.shape, generator=g))).contiguous()
        nll = (torch.tensor(WC)[None, :, None, None] * (pred - target).abs()).sum() / B
        dstate = D.init_state(DCFG, 3)
        g_loss = -torch.mean(D.forward_host(dstate, pred, training=True))
        last = sdt["decoder.conv_out.weight"]
        d_weight = D.adaptive_weight_host(torch.autograd.grad(nll, last, retain_graph=True)[0],
                                          torch.autograd.grad(g_loss, last, retain_graph=True)[0], 0.5)
        grads = dict(zip(keys, torch.autograd.grad(nll + d_weight * g_loss, [sdt[k] for k in keys])))
        # the discriminator's step (the reference's second optimizer; its first step here)
        dp = {k: torch.nn.Parameter(v.clone()) for k, v in dstate.items() if not k.endswith(D.BUFFER_SUFFIXES)}
        buffers = {k: v.clone() for k, v in dstate.items() if k.endswith(D.BUFFER_SUFFIXES)}
        opt = torch.optim.Adam(list(dp.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
        st = dict(dp, **buffers)
        buffers2 = {k: v.clone() for k, v in buffers.items()}
        D.forward_host(st, pred.detach(), True, False, buffers2)      # (the generator's pass moved the running statistics first)
        d_loss = D.hinge_d_loss_host(D.forward_host(st, target, True, False, buffers2), D.forward_host(st, pred.detach(), True, False, buffers2))
        d_loss.backward()
        opt.step()
        _ADV.update(cfg=cfg, B=B, lr=lr, sd=sd, z=z, target=target, pred=pred.detach(), dstate=dstate, d_weight=float(d_weight),
                    g_loss=float(g_loss.detach()), grads=grads, d_loss=float(d_loss.detach()),
                    dparams={k: v.detach() for k, v in dp.items()}, dbuffers=buffers2)
    return _ADV


def adversarial_figures(det=False):
    """One adversarial train_step of VAEDecoderTrainer at SMALL -> the figures STEP_GATES is about."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer
    o = adv_case()
    disc = D.PatchDiscriminator(state=o["dstate"], lr=o["lr"], deterministic=det)
    tr = VAEDecoderTrainer(o["cfg"], o["sd"], lr=o["lr"], discriminator=disc, disc_start=0, deterministic=det)
    assert tr.adversarial()
    snap = {}
    step = tr.optimizer_step

    def keep_then_step():
        snap.update({n: tr.g[n].cpu().clone() for n in tr.names})
        return step()
    tr.optimizer_step = keep_then_step
    loss = tr.train_step(o["z"].cuda(), o["target"].cuda())
    torch.cuda.synchronize()
    assert tr.global_step == 1 and disc.global_step == 1
    w, n, a = _param_errors(snap, o["grads"], tr.names)
    got = disc.state_dict()
    names = disc.names
    d = torch.cat([(got[k] - o["dparams"][k]).reshape(-1) for k in names]).abs()
    upd = torch.cat([(o["dparams"][k] - o["dstate"][k]).reshape(-1) for k in names])
    d_loss, mean_real, mean_fake = (float(v) for v in tr.last_disc)
    return dict(d_weight=abs(float(tr.last_d_weight) - o["d_weight"]) / o["d_weight"], g_loss=abs(float(tr.last_g_loss) - o["g_loss"]) / abs(o["g_loss"]),
                grad_worst=w, grad_worst_name=n, grad_all=a, d_loss=abs(d_loss - o["d_loss"]) / o["d_loss"],
                adam_beyond_half_step=float((d > 0.5 * o["lr"]).float().mean()), adam_rel=float(d.norm() / upd.norm()),
                running=max(U.rel(got[k], o["dbuffers"][k]) for k in got if k.endswith(("running_mean", "running_var"))),
                nbt=int(got["main.3.num_batches_tracked"]), loss=float(loss), mean_real=mean_real, mean_fake=mean_fake)


STEP_KEYS = ("d_weight", "g_loss", "grad_worst", "grad_all", "d_loss", "running", "adam_beyond_half_step", "adam_rel")
# measured (worst of three): d_weight 0.00228, g_loss 0.0017, grad_worst 0.0299 (decoder.up_blocks.0.upsamplers.0.conv.bias), grad_all
# 0.0249, d_loss 3.07e-05, running 0.00197, adam_beyond_half_step 0.0151, adam_rel 0.244.  The VAE's gradients sit where
# tests/test_vae_training_gpu.py's do (its SMALL gates: 3.9e-2 / 1.5e-2; the whole-buffer figure is higher here because the generator
# term's gradient has passed through the discriminator's bf16 convs as well).  The Adam figures are the first step's: Adam's first update
# is lr sign(g), so a parameter whose gradient changes sign under the roundings above lands 2 lr away -- 1.5 % of them do, and
# |difference| / |update| = sqrt(4 x 0.015) = 0.245 is that same count, not a second error.
STEP_GATES = dict(d_weight=0.0046, g_loss=0.0034, grad_worst=0.06, grad_all=0.05, d_loss=6.2e-05, running=0.004,
                  adam_beyond_half_step=0.031, adam_rel=0.49)


def test_adversarial_step_matches_autograd_and_adam():
    """d_weight against adaptive_weight_host; every VAE parameter gradient against autograd of nll + d_weight g_loss; the discriminator
    after its step against torch Adam (the two figures of tests/test_vae_training_gpu.py::test_train_steps_follow_adam: the share of
    parameters beyond half a step, |difference| / |update|); gates and measured values at STEP_GATES."""
    fig = adversarial_figures()
    print("adversarial step at SMALL: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
    assert fig["nbt"] == 3                                             # the generator's pass, then real, then fake
    bad = {k: (fig[k], STEP_GATES[k]) for k in STEP_KEYS if not fig[k] <= STEP_GATES[k]}
    assert not bad, bad


def _vae_bits(tr):
    return [t.cpu().clone() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


def _vae_batch(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    f = cfg.downscale
    images = torch.rand(B, cfg.in_channels, *cfg.sample_size, generator=g)
    noise = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
    return images, noise


@pytest.mark.parametrize("which", ["decoder", "all"])
def test_without_a_discriminator_and_before_disc_start_the_step_is_todays(which):
    """Three deterministic steps: the trainer as it always was, the trainer with discriminator=None spelled out, and the trainer with a
    discriminator whose phase has not started -- the same parameter, moment and loss bits; the waiting discriminator is never run."""
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    o = adv_case()
    cfg, sd = o["cfg"], o["sd"]
    batches = [_vae_batch(cfg, 2, 80 + i) for i in range(3)]
    runs = []
    for kw in ({}, dict(discriminator=None, disc_start=0), dict(discriminator="later", disc_start=3)):
        disc = None
        if kw.get("discriminator") == "later":
            disc = kw["discriminator"] = D.PatchDiscriminator(state=o["dstate"], deterministic=True)
        if which == "all":
            tr = VAETrainer(cfg, sd, lr=1e-3, deterministic=True, **kw)
            losses = [float(tr.train_step(x.cuda(), noise=n.cuda())) for x, n in batches]
        else:
            tr = VAEDecoderTrainer(cfg, sd, lr=1e-3, deterministic=True, **kw)
            losses = [float(tr.train_step(n.cuda(), x.cuda())) for x, n in batches]
        runs.append((losses, _vae_bits(tr)))
        assert tr.last_disc is None and tr.last_g_loss is None and tr.last_d_weight is None
        if disc is not None:
            assert tr.adversarial()                                    # three steps taken: the fourth would be the first adversarial one
            assert disc.global_step == 0 and int(disc.buffers["main.3.num_batches_tracked"]) == 0
            assert torch.equal(disc.params.cpu(), torch.cat([o["dstate"][n].reshape(-1) for n in disc.names]))
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert all(torch.equal(x, y) for x, y in zip(runs[0][1], other[1]))


def test_saved_state_continues_bit_identically_across_the_phase_boundary(tmp_path):
    from rangeldm_amd.vae_training import VAETrainer
    o = adv_case()
    cfg, sd = o["cfg"], o["sd"]
    batches = [_vae_batch(cfg, 2, 90 + i) for i in range(4)]

    def make(seed):
        disc = D.PatchDiscriminator(DCFG, seed=seed, lr=1e-3, deterministic=True)
        return VAETrainer(cfg, sd, lr=1e-3, deterministic=True, discriminator=disc, disc_start=2)
    a = make(3)
    for x, n in batches[:1]:
        a.train_step(x.cuda(), noise=n.cuda())
    path = str(tmp_path / "state.pt")
    a.save_state(path)
    for x, n in batches[1:]:
        a.train_step(x.cuda(), noise=n.cuda())                         # step 2 plain, steps 3 and 4 adversarial
    assert a.last_disc is not None and a.discriminator.global_step == 4
    assert int(a.discriminator.buffers["main.3.num_batches_tracked"]) == 6
    b = make(3)
    b.load_state(path)
    VAE_KEYS = {"params", "exp_avg", "exp_avg_sq", "global_step", "names"}
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert b.global_step == 1 and set(st) == VAE_KEYS | {"discriminator"} and set(st["discriminator"]) == U.STATE_KEYS
    for x, n in batches[1:]:
        b.train_step(x.cuda(), noise=n.cuda())
    for x, y in zip(_vae_bits(a) + _vae_bits(a.discriminator), _vae_bits(b) + _vae_bits(b.discriminator)):
        assert torch.equal(x, y)
    assert all(torch.equal(a.discriminator.buffers[k], b.discriminator.buffers[k]) for k in a.discriminator.buffers)
    assert float(a.last_d_weight) == float(b.last_d_weight) and float(a.last_g_loss) == float(b.last_g_loss)
    # a file written without a discriminator has no such key and keeps loading, also into a trainer that has one
    plain = VAETrainer(cfg, sd, lr=1e-3, deterministic=True)
    plain.train_step(batches[0][0].cuda(), noise=batches[0][1].cuda())
    plain.save_state(path)
    assert set(torch.load(path, map_location="cpu", weights_only=True)) == VAE_KEYS
    c = make(5)
    before = c.discriminator.params.clone()
    c.load_state(path)
    assert c.global_step == 1 and torch.equal(c.params, plain.params) and torch.equal(c.discriminator.params, before)


def test_command_line_runs_the_adversarial_phase(tmp_path, capsys):
    """python -m rangeldm_amd.train_vae --discriminator patchgan, in process: the new JSON keys from the first adversarial step on,
    OUT/discriminator.pt beside OUT/vae/; without the option the lines and the files are what they were."""
    from rangeldm_amd import train_vae as CLI
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae_training import save_vae_dir
    from tests.test_vae_training_gpu import TALL
    cfg = TALL
    sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
    src, out, out2 = tmp_path / "src", tmp_path / "out", tmp_path / "out2"
    save_vae_dir(str(src), cfg, sd)
    base = ["--weights", str(src), "--steps", "3", "--batch-size", "2", "--lr", "1e-3", "--log-every", "1", "--seed", "4"]
    CLI.main(base + ["--out", str(out), "--discriminator", "patchgan", "--disc-start", "1", "--disc-weight", "0.5"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [1, 2, 3]
    new = {"g_loss", "d_weight", "disc_loss", "logits_real", "logits_fake"}
    assert set(lines[0]) == {"step", "loss", "mae"}
    for l in lines[1:]:
        assert set(l) == {"step", "loss", "mae"} | new and all(np.isfinite(l[k]) for k in new)
        assert 0.0 <= l["d_weight"] <= 0.5 * 1e4 and l["disc_loss"] > 0
    assert (out / "vae").is_dir() and (out / "discriminator.pt").is_file()
    st = torch.load(str(out / "discriminator.pt"), map_location="cpu", weights_only=True)
    assert st["global_step"] == 3 and list(st["names"]) == D.trainable_names() and int(st["buffers"]["main.3.num_batches_tracked"]) == 6
    again = D.PatchDiscriminator(device="cuda")
    again.load_state(str(out / "discriminator.pt"))
    CLI.main(base + ["--out", str(out2)])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert all(set(l) == {"step", "loss", "mae"} for l in lines) and not (out2 / "discriminator.pt").exists()
