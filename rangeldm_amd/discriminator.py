"""The PatchGAN discriminator of the VAE's adversarial phase on MI355X: the reference's plain `NLayerDiscriminator`
(vae/sgm/modules/autoencoding/lpips/model/model.py:18-89; vae/configs/nuscenes.yaml selects it with ndf = 64, n_layers = 3) and the
discriminator half of `GeneralLPIPSWithDiscriminator` (hinge loss, a second Adam).

    main.0   Conv2d(in, ndf, 4, stride 2, pad 1) + bias, LeakyReLU(0.2)
    main.2   Conv2d(ndf, 2 ndf, 4, 2, 1), main.3 BatchNorm2d, LeakyReLU(0.2)          (n_layers - 1 of these, widths doubling up to 8 ndf)
    main.5   Conv2d(2 ndf, 4 ndf, 4, 2, 1), main.6 BatchNorm2d, LeakyReLU(0.2)
    main.8   Conv2d(4 ndf, 8 ndf, 4, stride 1, pad 1), main.9 BatchNorm2d, LeakyReLU(0.2)
    main.11  Conv2d(8 ndf, 1, 4, 1, 1) + bias                                          one logit per patch

The padding is ZERO padding on both axes: W does not wrap in this network, unlike every other conv of the library.  BatchNorm runs in
training mode (batch statistics, running averages, num_batches_tracked) whenever the reference's does.

`PatchDiscriminator` drives the HIP kernels of rangeldm_amd/csrc/train_disc.hip (rldm_train_disc_*) from its own walk over the
layers, on `FlatParameters`' flat buffers (tape.py); `forward_host` restates the network in torch functional ops (autograd-capable,
optionally with the conv operands rounded to bf16 where the kernels round) and is the tests' reference.  The range-guided Meta-Kernel
network that vae/configs/kitti360.yaml selects is metakernel.py's: this module's walk, BatchNorm, LeakyReLU, loss kernels, optimizer
step and state handling around its own layer.  Not built: its
variant 2 (NLayerDiscriminatorMetaKernel2), `vanilla_d_loss`, ActNorm, gradient exchange between ranks.  (`disc_bev`, the PatchGAN on
the BEV volume of the reconstruction, is the VAE trainers': vae_training.py.)  No torch autograd
and no torch compute ops on the device path; no CPU fallback."""
import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import train_ops as T
from .tape import FlatParameters

BN_EPS, BN_MOMENTUM, SLOPE = 1e-5, 0.1, 0.2
SGM_PREFIX = "loss.discriminator."


@dataclass(frozen=True)
class DiscriminatorConfig:
    in_channels: int = 2
    ndf: int = 64
    n_layers: int = 3


def _cfg(config):
    if config is None:
        return DiscriminatorConfig()
    return config if isinstance(config, DiscriminatorConfig) else DiscriminatorConfig(**config)


def pyramid(cfg):
    """(name `main.K`, cin, cout, stride, bn `main.K+1` or None, act) of the layers in forward order: the widths and strides that the
    PatchGAN and the Meta-Kernel network (whose config extends this one) share."""
    yield "main.0", cfg.in_channels, cfg.ndf, 2, None, True
    mult = 1
    for n in range(1, cfg.n_layers + 1):
        prev, mult = mult, min(2 ** n, 8)
        k = 2 + 3 * (n - 1)
        yield f"main.{k}", cfg.ndf * prev, cfg.ndf * mult, 2 if n < cfg.n_layers else 1, f"main.{k + 1}", True
    yield f"main.{2 + 3 * cfg.n_layers}", cfg.ndf * mult, 1, 1, None, False


def layer_specs(cfg):
    """The convs in forward order: dicts with name (`main.K`), cin, cout, stride, bias (bool), bn (`main.K+1` or None), act (bool).
    A conv in front of a BatchNorm has no bias."""
    return [dict(name=name, cin=cin, cout=cout, stride=stride, bias=bn is None, bn=bn, act=act)
            for name, cin, cout, stride, bn, act in pyramid(_cfg(cfg))]


def param_shapes(cfg=None):
    """Every key of the reference module's state_dict(), in its order: parameters and BatchNorm buffers."""
    shapes = OrderedDict()
    for L in layer_specs(cfg):
        shapes[L["name"] + ".weight"] = (L["cout"], L["cin"], 4, 4)
        if L["bias"]:
            shapes[L["name"] + ".bias"] = (L["cout"],)
        if L["bn"]:
            for k in ("weight", "bias", "running_mean", "running_var"):
                shapes[f"{L['bn']}.{k}"] = (L["cout"],)
            shapes[L["bn"] + ".num_batches_tracked"] = ()
    return shapes


BUFFER_SUFFIXES = (".running_mean", ".running_var", ".num_batches_tracked")


def trainable_names(cfg=None):
    return [k for k in param_shapes(cfg) if not k.endswith(BUFFER_SUFFIXES)]


def output_size(cfg, W, H):
    """(Wo, Ho) of the logits for a (W, H) input, for either network (the Meta-Kernel's W is counted on its W + 2 wrapped columns:
    the same extents as with zero padding)."""
    for _, _, _, stride, _, _ in pyramid(_cfg(cfg)):
        W, H = conv_out_size(W, H, stride)
    return W, H


def init_state(cfg=None, seed=0):
    """The reference's initialisation (`weights_init`: conv weights N(0, 0.02), BatchNorm weights N(1, 0.02), BatchNorm biases 0; conv
    biases keep torch's default U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))) from a seeded host generator; fresh BatchNorm buffers."""
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for L in layer_specs(cfg):
        sd[L["name"] + ".weight"] = torch.randn((L["cout"], L["cin"], 4, 4), generator=g) * 0.02
        if L["bias"]:
            bound = 1.0 / float(np.sqrt(L["cin"] * 16))
            sd[L["name"] + ".bias"] = (torch.rand((L["cout"],), generator=g) * 2 - 1) * bound
        if L["bn"]:
            sd[L["bn"] + ".weight"] = 1.0 + torch.randn((L["cout"],), generator=g) * 0.02
            sd[L["bn"] + ".bias"] = torch.zeros(L["cout"])
            sd[L["bn"] + ".running_mean"] = torch.zeros(L["cout"])
            sd[L["bn"] + ".running_var"] = torch.ones(L["cout"])
            sd[L["bn"] + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return sd


def pick_discriminator_state(sgm_state_dict, prefix=SGM_PREFIX):
    """The discriminator's entries of a trained sgm checkpoint's state dict -- `loss.discriminator.*`, also behind an outer prefix such
    as `first_stage_model.` -- with everything up to and including the prefix stripped.  (The VAE converter in checkpoint.py drops
    them: an inference VAE has no use for them.)"""
    out = OrderedDict()
    for k, v in sgm_state_dict.items():
        i = k.find(prefix)
        if i == 0 or (i > 0 and k[i - 1] == "."):
            out[k[i + len(prefix):]] = v
    if not out:
        raise KeyError(f"no `{prefix}*` entries in the state dict")
    return out


def config_from_state(state):
    """The DiscriminatorConfig a state dict with the reference's keys was built with."""
    w0 = state["main.0.weight"]
    convs = sorted(int(k.split(".")[1]) for k in state if k.endswith(".weight") and len(state[k].shape) == 4)
    return DiscriminatorConfig(in_channels=int(w0.shape[1]), ndf=int(w0.shape[0]), n_layers=len(convs) - 2)


def grad_sample_indices(numel, cap=1024):
    """The elements of a flattened gradient that tests/golden/discriminator.npz records: all of them up to `cap`, else `cap` evenly
    spaced ones (first and last included) -- the file stays small, the gradient's L2 norm over ALL elements is recorded beside them."""
    return np.arange(numel, dtype=np.int64) if numel <= cap else np.linspace(0, numel - 1, cap).round().astype(np.int64)


# ---- host statements ---------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Bf16Conv(torch.autograd.Function):
    """conv2d whose three GEMMs see bf16-rounded operands, as the kernels': forward r(x) * r(w); data gradient r(dy) * r(w); weight
    gradient r(dy) * r(x); the bias sum takes dy as it is."""

    @staticmethod
    def forward(ctx, x, w, bias, stride):
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.has_bias = stride, bias is not None
        return F.conv2d(_bf16(x), _bf16(w), bias, stride=stride, padding=1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = _bf16(dy)
        dx = torch.nn.grad.conv2d_input(x.shape, _bf16(w), r, stride=ctx.stride, padding=1)
        dw = torch.nn.grad.conv2d_weight(_bf16(x), w.shape, r, stride=ctx.stride, padding=1)
        return dx, dw, (dy.sum((0, 2, 3)) if ctx.has_bias else None), None


def batchnorm_running_host(h, state, buffers, bn, training):
    """F.batch_norm of layer `bn` (its weight and bias from `state`); training: batch statistics, and the running statistics and
    the counter updated IN `buffers`."""
    rm, rv = buffers[bn + ".running_mean"], buffers[bn + ".running_var"]
    rm_, rv_ = rm.detach().to(h.dtype, copy=True), rv.detach().to(h.dtype, copy=True)     # (autograd keeps what it is given)
    h = F.batch_norm(h, rm_, rv_, state[bn + ".weight"].to(h.dtype), state[bn + ".bias"].to(h.dtype), training, BN_MOMENTUM, BN_EPS)
    if training:
        rm.copy_(rm_)
        rv.copy_(rv_)
        buffers[bn + ".num_batches_tracked"] += 1
    return h


def forward_host(state, x, training=True, bf16=False, buffers=None):
    """The network in plain torch: x (B, in_channels, W, H) -> logits (B, 1, Wo, Ho), differentiable in x and in every tensor of
    `state` that requires grad.  training: BatchNorm uses batch statistics and updates the running statistics IN `buffers` (a dict with
    the `*.running_mean / running_var / num_batches_tracked` keys; None: copies of state's, dropped).  bf16: every conv's operands are
    rounded to bf16 where the kernels round (forward and both gradients); everything else stays in x's dtype."""
    state = {k: torch.as_tensor(v) for k, v in state.items()}
    cfg = config_from_state(state)
    if buffers is None:
        buffers = {k: v.detach().clone() for k, v in state.items() if k.endswith(BUFFER_SUFFIXES)}
    h = x
    for L in layer_specs(cfg):
        w = state[L["name"] + ".weight"].to(h.dtype)
        b = state[L["name"] + ".bias"].to(h.dtype) if L["bias"] else None
        h = _Bf16Conv.apply(h, w, b, L["stride"]) if bf16 else F.conv2d(h, w, b, stride=L["stride"], padding=1)
        if L["bn"]:
            h = batchnorm_running_host(h, state, buffers, L["bn"], training)
        if L["act"]:
            h = F.leaky_relu(h, SLOPE)
    return h


def hinge_d_loss_host(logits_real, logits_fake, factor=1.0):
    """vqperceptual.hinge_d_loss times factor (torch, differentiable)."""
    return factor * 0.5 * (torch.mean(F.relu(1.0 - logits_real)) + torch.mean(F.relu(1.0 + logits_fake)))


def hinge_host(real, fake, factor=1.0):
    """rldm_train_disc_hinge in numpy fp64 on fp32 logits: -> (out [3] = (loss, mean real, mean fake), dreal, dfake fp32)."""
    real, fake = np.asarray(real, np.float32).reshape(-1), np.asarray(fake, np.float32).reshape(-1)
    n = real.size
    a, b = np.float32(1) - real, np.float32(1) + fake
    g = np.float32(0.5 * float(np.float32(factor)) / n)
    out = np.array([0.5 * float(np.float32(factor)) * (np.maximum(a, 0).astype(np.float64).sum() + np.maximum(b, 0).astype(np.float64).sum()) / n,
                    real.astype(np.float64).sum() / n, fake.astype(np.float64).sum() / n])
    return out, np.where(a > 0, -g, np.float32(0)).astype(np.float32), np.where(b > 0, g, np.float32(0)).astype(np.float32)


def adaptive_weight_host(nll_grads, g_grads, disc_weight=0.5):
    """GeneralLPIPSWithDiscriminator.calculate_adaptive_weight on the two gradients of the last layer (any float dtype)."""
    w = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
    return torch.clamp(w, 0.0, 1e4).detach() * disc_weight


def batchnorm_host(x, gamma, beta, running_mean=None, running_var=None, training=True, dy=None):
    """rldm_train_disc_bn_forward / _backward stated in numpy fp64.  x [M][C] (any leading shape, channels last).  -> dict with y, mean,
    var (biased), rstd, running_mean, running_var (updated with the UNBIASED variance when training) and, given dy: dx, dgamma, dbeta.
    LeakyReLU's gradient at z == 0 is the slope-0.2 side."""
    x = np.asarray(x, np.float64)
    C_ = x.shape[-1]
    x2 = x.reshape(-1, C_)
    M = x2.shape[0]
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    out = {}
    if training:
        if M < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean = x2.sum(0) / M
        var = np.maximum((x2 * x2).sum(0) / M - mean * mean, 0.0)
        if running_mean is not None:
            out["running_mean"] = (1 - BN_MOMENTUM) * np.asarray(running_mean, np.float64) + BN_MOMENTUM * mean
            out["running_var"] = (1 - BN_MOMENTUM) * np.asarray(running_var, np.float64) + BN_MOMENTUM * var * M / (M - 1)
    else:
        mean, var = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    xh = (x2 - mean) * rstd
    z = xh * gamma + beta
    out.update(y=np.where(z > 0, z, SLOPE * z).reshape(x.shape), mean=mean, var=var, rstd=rstd)
    if dy is not None:
        dz = np.asarray(dy, np.float64).reshape(-1, C_) * np.where(z > 0, 1.0, SLOPE)
        s1, s2 = dz.sum(0), (dz * xh).sum(0)
        out.update(dbeta=s1, dgamma=s2, dx=((gamma * rstd) * (dz - s1 / M - xh * s2 / M)).reshape(x.shape))
    return out


# ---- the kernels (device fp32, NHWC) ---------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s(t):
    return _lib.stream_ptr(t.device)


def _workspace(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def conv_desc(x_shape, N, stride):
    """The desc of the FORWARD conv for an input (B, W, H, Cin); ValueError where the library has no instance."""
    d = _lib.TrainDiscConvDescC()
    d.B, d.Win, d.Hin, d.Cin = (int(v) for v in x_shape)
    d.N, d.stride = int(N), int(stride)
    if not _lib.lib().rldm_train_disc_conv_ok(C.byref(d)):
        raise ValueError(f"no 4x4 discriminator conv instance for input {tuple(x_shape)} (NHWC), N = {N}, stride {stride}: Cin is 2 or a "
                         f"multiple of 16, N is 1 or a multiple of 16, stride 1 or 2, extents >= 2")
    return d


def conv_out_size(W, H, stride):
    return (W - 2) // stride + 1, (H - 2) // stride + 1


def conv4(x, w_packed, N, stride, bias=None):
    """x (B, W, H, Cin) -> (B, Wo, Ho, N): 4x4, zero padding 1 on both axes (no wrap).  w_packed: train_ops.pack_weights(w, 16)[0]."""
    d = conv_desc(x.shape, N, stride)
    Wo, Ho = conv_out_size(x.shape[1], x.shape[2], stride)
    y = T.empty((x.shape[0], Wo, Ho, N), x)
    _lib.check(_lib.lib().rldm_train_disc_conv(C.byref(d), _p(x), _p(w_packed), _p(bias), _p(y), _s(x)), "rldm_train_disc_conv")
    return y


def conv4_dgrad(dy, w_transposed, x_shape, stride):
    """dy (B, Wo, Ho, N) -> dx of shape x_shape (B, W, H, Cin).  w_transposed: pack_weights(w, 16)[1]."""
    d = conv_desc(x_shape, dy.shape[3], stride)
    if tuple(dy.shape[:3]) != (x_shape[0], *conv_out_size(x_shape[1], x_shape[2], stride)):
        raise ValueError(f"dy {tuple(dy.shape)} is not the output of a stride-{stride} conv over {tuple(x_shape)}")
    dx = T.empty(tuple(x_shape), dy)
    _lib.check(_lib.lib().rldm_train_disc_conv_dgrad(C.byref(d), _p(dy), _p(w_transposed), _p(dx), _s(dy)), "rldm_train_disc_conv_dgrad")
    return dx


def conv4_wgrad(dy, x, dw, stride, dbias=None):
    """dw (N, Cin, 4, 4) += dy (x) x; dbias (N,) += the column sums of dy.  Both are views into zeroed gradient buffers."""
    d = conv_desc(x.shape, dy.shape[3], stride)
    nbytes = _lib.lib().rldm_train_disc_wgrad_workspace(C.byref(d))
    ws = _workspace(nbytes, x)
    _lib.check(_lib.lib().rldm_train_disc_wgrad(C.byref(d), _p(dy), _p(x), _p(dw), _p(dbias), _p(ws), ws.numel(), _s(x)),
               "rldm_train_disc_wgrad")


def bn_lrelu_forward(x, gamma, beta, running_mean, running_var, num_batches_tracked, training=True):
    """-> (y, save [2 C] = (mean | rstd)).  Training: batch statistics; the running statistics and the counter are updated in place."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    if training and M < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    y, save = torch.empty_like(x), T.empty((2 * Cc,), x)
    ws = _workspace(_lib.lib().rldm_train_disc_bn_workspace(M, Cc), x)
    _lib.check(_lib.lib().rldm_train_disc_bn_forward(_p(x), M, Cc, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                                     _p(num_batches_tracked), 1 if training else 0, _p(save), _p(y), _p(ws),
                                                     ws.numel(), _s(x)), "rldm_train_disc_bn_forward")
    return y, save


def bn_lrelu_backward(x, dy, save, gamma, beta, dgamma=None, dbeta=None):
    """-> dx; dgamma / dbeta (views into zeroed gradient buffers) += their gradients, or None for the input gradient alone."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    dx = torch.empty_like(x)
    ws = _workspace(_lib.lib().rldm_train_disc_bn_workspace(M, Cc), x)
    _lib.check(_lib.lib().rldm_train_disc_bn_backward(_p(x), _p(dy), _p(save), M, Cc, _p(gamma), _p(beta), _p(dx), _p(dgamma), _p(dbeta),
                                                      _p(ws), ws.numel(), _s(x)), "rldm_train_disc_bn_backward")
    return dx


def lrelu(x):
    y = torch.empty_like(x)
    _lib.check(_lib.lib().rldm_train_disc_lrelu(_p(x), None, _p(y), x.numel(), 0, _s(x)), "rldm_train_disc_lrelu")
    return y


def lrelu_backward(x, dy):
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().rldm_train_disc_lrelu(_p(x), _p(dy), _p(dx), x.numel(), 1, _s(x)), "rldm_train_disc_lrelu")
    return dx


def _partials(n, rows, like):
    return torch.empty(rows * ((n + 255) // 256), dtype=torch.float64, device=like.device)


def hinge(real, fake, factor=1.0):
    """-> (out: float64 (3,) device = (factor * hinge_d_loss, mean real, mean fake), dreal, dfake).  No host sync."""
    if real.shape != fake.shape:
        raise ValueError(f"hinge: logits {tuple(real.shape)} and {tuple(fake.shape)}")
    n = real.numel()
    out = torch.empty(3, dtype=torch.float64, device=real.device)
    dreal, dfake, part = torch.empty_like(real), torch.empty_like(fake), _partials(n, 3, real)
    _lib.check(_lib.lib().rldm_train_disc_hinge(_p(real), _p(fake), n, float(factor), _p(dreal), _p(dfake), _p(out), _p(part), _s(real)),
               "rldm_train_disc_hinge")
    return out, dreal, dfake


def generator_loss(fake):
    """-> (g_loss = -mean(fake): 0-d float64 device tensor, dfake = -1 / n)."""
    n = fake.numel()
    out = torch.empty((), dtype=torch.float64, device=fake.device)
    dfake, part = torch.empty_like(fake), _partials(n, 1, fake)
    _lib.check(_lib.lib().rldm_train_disc_generator(_p(fake), n, _p(dfake), _p(out), _p(part), _s(fake)), "rldm_train_disc_generator")
    return out, dfake


def adaptive_mix(dnll, dg, sq_nll, sq_g, disc_weight, disc_factor):
    """-> (dpred = dnll + (d_weight disc_factor) dg, d_weight: 0-d float64 device tensor) with d_weight = clamp(sqrt(sq_nll) / (sqrt(sq_g)
    + 1e-4), 0, 1e4) disc_weight read from the two device scalars."""
    if dnll.shape != dg.shape:
        raise ValueError(f"adaptive_mix: gradients {tuple(dnll.shape)} and {tuple(dg.shape)}")
    dpred = torch.empty_like(dnll)
    dw = torch.empty((), dtype=torch.float64, device=dnll.device)
    _lib.check(_lib.lib().rldm_train_disc_adaptive_mix(_p(dnll), _p(dg), _p(sq_nll), _p(sq_g), float(disc_weight), float(disc_factor),
                                                       _p(dpred), _p(dw), dnll.numel(), _s(dnll)), "rldm_train_disc_adaptive_mix")
    return dpred, dw




# ---- the network on the tape -------------------------------------------------------------------------------------------------------
class _Pass:
    """One forward pass: per layer (spec, layer input, layer output, BatchNorm statistics, what the layer saved), the logits, the
    mode.  A layer may hang per-pass extras on it (the Meta-Kernel's range image)."""

    def __init__(self, training):
        self.rec, self.logits, self.training = [], None, training


class PatchDiscriminator(FlatParameters):
    """Owns the walk over `specs` -- layer, then BatchNorm + LeakyReLU / LeakyReLU / nothing, and the mirror image backwards --, the
    losses, the optimizer step and the state.  What a layer is stands in `_layer_forward` / `_layer_backward` alone: here the 4x4
    zero-padded conv, in metakernel.MetaKernelDiscriminator the Meta-Kernel layer."""
    _state_name = "discriminator state"

    def __init__(self, config=None, state=None, seed=0, device="cuda", lr=4.5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 deterministic=False):
        """state: a dict with the reference's keys (init_state, or pick_discriminator_state of an sgm checkpoint); None:
        init_state(config, seed).  The optimizer's defaults are the reference's second Adam (base_learning_rate 4.5e-6, no decay).
        deterministic: every kernel of this object runs in the library's deterministic mode (rldm_train_deterministic), as on the
        other trainers: the same inputs give the same parameter bits."""
        cfg = _cfg(config) if state is None or config is not None else config_from_state(state)
        state = state if state is not None else init_state(cfg, seed)
        # tiled=False: the tiled packer stages 64 x 64 x taps weights in LDS and is sized for 9 taps
        self._build(cfg, state, layer_specs(cfg), param_shapes(cfg), trainable_names(cfg), BUFFER_SUFFIXES, device,
                    dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=None), deterministic, tiled=False)

    def _build(self, cfg, state, specs, shapes, names, buffer_suffixes, device, hp, deterministic, **store):
        """shapes: every key of the reference's state dict, in its order; names: the trainable ones; buffer_suffixes: the rest, loaded
        into `buffers` (BatchNorm's get their fresh values when `state` has none); store: FlatParameters' packing options."""
        self.cfg, self.specs, self.hp, self._keys = cfg, specs, hp, list(shapes)
        self._init_parameters(OrderedDict((n, shapes[n]) for n in names), names, state, device, deterministic=deterministic, **store)
        self.buffers = OrderedDict()
        for k, shape in shapes.items():
            if k.endswith(buffer_suffixes):
                v = state.get(k)
                if v is None:
                    if not k.endswith(BUFFER_SUFFIXES):
                        raise KeyError(f"the state dict has no buffer {k}")
                    v = torch.ones(shape) if k.endswith("running_var") else torch.zeros(shape)
                v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
                dt = torch.int64 if k.endswith("num_batches_tracked") else torch.float32
                self.buffers[k] = v.detach().to(dt).reshape(shape).clone().to(self.device)
        self._pass = None

    # ---- one layer --------------------------------------------------------------------------------------------
    def _layer_forward(self, ps, L, x):
        """-> (the layer's output, what its backward needs besides x)."""
        n = L["name"]
        return conv4(x, self.wf[n + ".weight"], L["cout"], L["stride"], self.p[n + ".bias"] if L["bias"] else None), None

    def _layer_backward(self, ps, L, x, dy, saved, params, want_input):
        """params: the layer's parameter gradients += theirs.  -> d / dx; None from the first layer unless want_input: the gradient
        of the network's input is wanted."""
        n = L["name"]
        if params:
            conv4_wgrad(dy, x, self.g[n + ".weight"], L["stride"], self.g[n + ".bias"] if L["bias"] else None)
        if L is self.specs[0] and not want_input:
            return None
        return conv4_dgrad(dy, self.wt[n + ".weight"], x.shape, L["stride"])

    # ---- forward ----------------------------------------------------------------------------------------------
    def _input(self, x, layout):
        x = x.to(self.device).float().contiguous()
        cin = self.cfg.in_channels
        if x.dim() != 4:
            raise ValueError(f"the discriminator takes a 4-d batch, not {tuple(x.shape)}")
        if layout is None:
            layout = "nchw" if x.shape[1] == cin else ("nhwc" if x.shape[3] == cin else None)
        if layout == "nchw" and x.shape[1] == cin:
            return T.pack_input(x, False)
        if layout == "nhwc" and x.shape[3] == cin:
            return x
        raise ValueError(f"input {tuple(x.shape)} has no axis of {cin} channels where layout {layout!r} puts it")

    def forward(self, x, training=True, layout=None):
        """x: (B, in_channels, W, H) or NHWC (B, W, H, in_channels) (layout None: NCHW if axis 1 has in_channels entries, else NHWC)
        -> the logits (B, Wo, Ho, 1) NHWC on the device.  training: BatchNorm takes batch statistics and updates the running ones
        (what the reference does in both of its uses); False: running statistics, nothing recorded for a backward."""
        with self._mode():
            h = self._input(x, layout)
            ps = _Pass(bool(training))
            for L in self.specs:
                xin = h
                y, saved = self._layer_forward(ps, L, xin)
                save = None
                if L["bn"]:
                    b = L["bn"]
                    h, save = bn_lrelu_forward(y, self.p[b + ".weight"], self.p[b + ".bias"], self.buffers[b + ".running_mean"],
                                               self.buffers[b + ".running_var"], self.buffers[b + ".num_batches_tracked"], training)
                elif L["act"]:
                    h = lrelu(y)
                else:
                    h = y
                ps.rec.append((L, xin, y, save, saved))
            ps.logits = h
            self._pass = ps
            return h

    def logits(self):
        """The last forward's logits as (B, 1, Wo, Ho)."""
        return T.unpack_output(self._pass.logits)

    # ---- backward ---------------------------------------------------------------------------------------------
    def _backward(self, ps, dlogits, params, want_input):
        if not ps.training:
            raise RuntimeError("the backward pass needs a training-mode forward (batch statistics)")
        if tuple(dlogits.shape) != tuple(ps.logits.shape):
            raise ValueError(f"dlogits {tuple(dlogits.shape)} for logits {tuple(ps.logits.shape)}")
        d = dlogits.contiguous()
        for L, xin, y, save, saved in reversed(ps.rec):
            if L["bn"]:
                b = L["bn"]
                d = bn_lrelu_backward(y, d, save, self.p[b + ".weight"], self.p[b + ".bias"],
                                      self.g[b + ".weight"] if params else None, self.g[b + ".bias"] if params else None)
            elif L["act"]:
                d = lrelu_backward(y, d)
            d = self._layer_backward(ps, L, xin, d, saved, params, want_input)
        return d

    def generator_loss(self):
        """The generator term of the last forward: (g_loss = -mean(logits), d g_loss / d logits)."""
        with self._mode():
            return generator_loss(self._pass.logits)

    def input_gradient(self, dlogits):
        """Replays the last forward's tape for d / d(input) alone: -> (B, W, H, in_channels) NHWC.  The parameter gradients are not
        touched (the generator's step differentiates through the discriminator, not into it)."""
        with self._mode():
            return self._backward(self._pass, dlogits, params=False, want_input=True)

    def backward(self, dlogits, ps=None):
        """The flat gradient buffer += d / d(parameters) of the last forward (no gradient to the input)."""
        with self._mode():
            self._backward(ps or self._pass, dlogits, params=True, want_input=False)

    def optimizer_step(self, step=None):
        """One Adam step on the flat buffers (then the bf16 operand copies are refreshed and the gradients zeroed).  step: the 1-based
        count used for the bias corrections (None: this object's own counter + 1)."""
        with self._mode():
            self.global_step = int(step) if step is not None else self.global_step + 1
            self._clip_adamw(self.hp["lr"])

    def discriminator_step(self, real, fake, factor=1.0, step=None):
        """forward(real), forward(fake) -- two passes, each with its own batch statistics and running-average update, as the
        reference's two calls --, the hinge loss times `factor`, the backward through both passes into the parameter gradients, one
        Adam step.  fake is used as it is (detached: nothing flows back to whoever made it).  -> (d_loss, mean logits real, mean
        logits fake): 0-d float64 device tensors, no host sync.  step: see optimizer_step (the VAE trainers pass their global_step: the
        reference's second optimizer steps from step 0 on, with zero gradients before disc_start, so its bias corrections do not
        restart there)."""
        with self._mode():
            lr_ = self.forward(real)
            pr = self._pass
            lf = self.forward(fake)
            pf = self._pass
            out, dreal, dfake = hinge(lr_, lf, factor)
            self._backward(pr, dreal, params=True, want_input=False)
            self._backward(pf, dfake, params=True, want_input=False)
            self.optimizer_step(step)
        return out[0], out[1], out[2]

    # ---- state ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Parameters and buffers under the reference's keys, in its order (host tensors)."""
        p = super().state_dict()
        return OrderedDict((k, p[k] if k in p else self.buffers[k].cpu().clone()) for k in self._keys)

    def state_payload(self):
        """Everything a resumed run needs: parameters, Adam moments, step counter, and the buffers (running statistics)."""
        return dict(super().state_payload(), buffers=OrderedDict((k, v.cpu()) for k, v in self.buffers.items()))

    def load_payload(self, st):
        super().load_payload(st)
        for k, v in st["buffers"].items():
            self.buffers[k].copy_(v)
