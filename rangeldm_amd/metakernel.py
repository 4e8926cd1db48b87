"""The range-guided Meta-Kernel discriminator of the VAE's adversarial phase on MI355X: the reference's
`NLayerDiscriminatorMetaKernel` (vae/sgm/modules/autoencoding/lpips/model/model.py:91-265), which vae/configs/kitti360.yaml selects
with `metakernel: True`, ndf = 64, n_layers = 3.  Losses and optimiser are the PatchGAN's (discriminator.py).

    main.0   MetaKernel(in -> ndf, stride 2), LeakyReLU(0.2)                        azi, inc
    main.2   MetaKernel(ndf -> 2 ndf, 2), main.3 BatchNorm2d, LeakyReLU(0.2)        2 azi, 2 inc      (n_layers - 1 of these)
    main.5   MetaKernel(2 ndf -> 4 ndf, 2), main.6 BatchNorm2d, LeakyReLU(0.2)      4 azi, 4 inc
    main.8   MetaKernel(4 ndf -> 8 ndf, stride 1), main.9 BatchNorm2d, LeakyReLU    8 azi, 8 inc
    main.11  MetaKernel(8 ndf -> 1, stride 1)                                       8 azi, 8 inc      one logit per patch

One layer, on x (B, C, W, H) and the range image r (B, 1, W, H) -- r = (input[:, :1] range_std + range_mean) / 10 at the network's
input, afterwards what the previous layer returned:
    for output pixel (wo, ho) and tap (i, j) (i: shift along H, j: shift along W) the source pixel is w = (s wo + j - 1) mod W
    (W WRAPS), h = s ho + i - 1; outside [0, H) x reads 0 and r reads 100.  Wo = (W - 2) // s + 1, Ho = (H - 2) // s + 1.
    r_c = r[(s wo + 1) mod W, s ho + 1]                      (tap (2, 2); returned as the next layer's r)
    pe0 = (r_tap cos_azi[i, j]) cos_inc[i, j] - r_c;  pe1 = (r_tap cos_azi[i, j]) sin_inc[i, j];  pe2 = r_tap sin_azi[i, j]
    m[c] = W2 lrelu_0.2(W1 pe + b1) + b2                      (mlp_coord.0: Linear(3, C), mlp_coord.2: Linear(C, C))
    out[n] = sum_{c,i,j} coov.weight[n, 16 c + 4 i + j] m[c](wo, ho, i, j) x[c](w, h) + coov.bias[n]
The four 4 x 4 tables are buffers of the state dict.  Every layer has its coov bias, also in front of a BatchNorm.

`MetaKernelDiscriminator` drives the HIP kernels of rangeldm_amd/csrc/train_meta.hip (rldm_train_meta_*) as the layers of
`PatchDiscriminator`'s walk (discriminator.py: its BatchNorm / LeakyReLU / loss kernels, optimizer step and state);
`forward_host` restates the network in torch (autograd-capable) and is the tests' reference, `layer_host` and its three pieces restate one layer with its gradients by hand.  The device keeps pe
(rows x 3), the source index of every row and the modulation m (rows x C, fp32: about 133 M elements = 0.53 GB per pass at batch 8,
1024 x 64) for the backward; a row is one (output pixel, tap) pair.  Not built: variant 2 (NLayerDiscriminatorMetaKernel2),
`log=True`, `disc_bev`, `vanilla_d_loss`, ActNorm.  No torch autograd and no torch compute ops on the device path; no CPU fallback."""
import ctypes as C
import math
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import discriminator as D
from . import train_ops as T
from .discriminator import (BUFFER_SUFFIXES, SLOPE, DiscriminatorConfig, PatchDiscriminator, _bf16, _p, _s, _workspace,  # noqa: F401
                            batchnorm_running_host, output_size)

TABLES = ("cos_azi", "sin_azi", "cos_inc", "sin_inc")           # the reference's registration order
TABLE_SUFFIXES = tuple("." + t for t in TABLES)
R_OUTSIDE = 100.0


@dataclass(frozen=True)
class MetaKernelConfig(DiscriminatorConfig):
    """in_channels, ndf, n_layers: the PatchGAN's (the same pyramid of widths and strides)."""
    azi: float = 0.00613592
    inc: float = 0.0074594
    range_mean: float = 20.0
    range_std: float = 40.0
    log: bool = False

    def __post_init__(self):
        if self.log:
            raise NotImplementedError("the Meta-Kernel discriminator's log = True range mapping is not built")


def _cfg(config):
    if config is None:
        return MetaKernelConfig()
    return config if isinstance(config, MetaKernelConfig) else MetaKernelConfig(**config)


def layer_specs(cfg=None):
    """The layers in forward order: dicts with name (`main.K`), cin, cout, stride, azi, inc, bn (`main.K+1` or None), act (bool)."""
    cfg = _cfg(cfg)
    out, azi, inc = [], cfg.azi, cfg.inc
    for name, cin, cout, stride, bn, act in D.pyramid(cfg):
        out.append(dict(name=name, cin=cin, cout=cout, stride=stride, azi=azi, inc=inc, bn=bn, act=act))
        azi, inc = azi * stride, inc * stride           # the angular step between neighbours doubles behind every stride-2 layer
    return out


def param_shapes(cfg=None):
    """Every key of the reference module's state_dict(), in its order: per layer the four tables, the MLP, coov; BatchNorm with its
    buffers."""
    shapes = OrderedDict()
    for L in layer_specs(cfg):
        n, c = L["name"], L["cin"]
        for t in TABLES:
            shapes[f"{n}.{t}"] = (1, 1, 1, 1, 4, 4)
        shapes[n + ".mlp_coord.0.weight"], shapes[n + ".mlp_coord.0.bias"] = (c, 3), (c,)
        shapes[n + ".mlp_coord.2.weight"], shapes[n + ".mlp_coord.2.bias"] = (c, c), (c,)
        shapes[n + ".coov.weight"], shapes[n + ".coov.bias"] = (L["cout"], 16 * c, 1, 1), (L["cout"],)
        if L["bn"]:
            for k in ("weight", "bias", "running_mean", "running_var"):
                shapes[f"{L['bn']}.{k}"] = (L["cout"],)
            shapes[L["bn"] + ".num_batches_tracked"] = ()
    return shapes


def trainable_names(cfg=None):
    return [k for k in param_shapes(cfg) if not k.endswith(BUFFER_SUFFIXES + TABLE_SUFFIXES)]


def make_tables(azi, inc):
    """The four (1, 1, 1, 1, 4, 4) tables as the reference builds them: fp32 cos / sin of fp32 [angle] * (shift - 2), indexed
    [shift_h, shift_w]; azi goes with shift_w, inc with shift_h."""
    a, b = torch.Tensor([azi]), torch.Tensor([inc])
    t = {k: torch.zeros(4, 4) for k in TABLES}
    for sh in range(4):
        for sw in range(4):
            t["cos_azi"][sh, sw] = torch.cos(a * (sw - 2))
            t["sin_azi"][sh, sw] = torch.sin(a * (sw - 2))
            t["cos_inc"][sh, sw] = torch.cos(b * (sh - 2))
            t["sin_inc"][sh, sw] = torch.sin(b * (sh - 2))
    return OrderedDict((k, t[k].reshape(1, 1, 1, 1, 4, 4)) for k in TABLES)


def init_state(cfg=None, seed=0):
    """The reference's initialisation from a seeded host generator: coov weights N(0, 0.02) and BatchNorm N(1, 0.02) / 0
    (`weights_init`); the Linears and coov.bias keep torch's default U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)); fresh BatchNorm
    buffers; the tables of make_tables."""
    g = torch.Generator().manual_seed(int(seed))
    u = lambda shape, fan_in: (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)      # noqa: E731
    sd = OrderedDict()
    for L in layer_specs(cfg):
        n, c, N = L["name"], L["cin"], L["cout"]
        for k, v in make_tables(L["azi"], L["inc"]).items():
            sd[f"{n}.{k}"] = v
        sd[n + ".mlp_coord.0.weight"], sd[n + ".mlp_coord.0.bias"] = u((c, 3), 3), u((c,), 3)
        sd[n + ".mlp_coord.2.weight"], sd[n + ".mlp_coord.2.bias"] = u((c, c), c), u((c,), c)
        sd[n + ".coov.weight"] = torch.randn((N, 16 * c, 1, 1), generator=g) * 0.02
        sd[n + ".coov.bias"] = u((N,), 16 * c)
        if L["bn"]:
            sd[L["bn"] + ".weight"] = 1.0 + torch.randn((N,), generator=g) * 0.02
            sd[L["bn"] + ".bias"] = torch.zeros(N)
            sd[L["bn"] + ".running_mean"] = torch.zeros(N)
            sd[L["bn"] + ".running_var"] = torch.ones(N)
            sd[L["bn"] + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return sd


def config_from_state(state, range_mean=20.0, range_std=40.0):
    """The MetaKernelConfig a state dict with the reference's keys was built with.  The angles are read back from the first layer's
    sine tables (sin(azi) at shift_w = 3, sin(inc) at shift_h = 3), so they are the fp32 values' arcsines; the network itself only ever
    uses the tables.  range_mean / range_std are not in a state dict."""
    w1 = torch.as_tensor(state["main.0.mlp_coord.0.weight"])
    coovs = [k for k in state if k.endswith(".coov.weight")]
    sa = torch.as_tensor(state["main.0.sin_azi"]).reshape(4, 4)
    si = torch.as_tensor(state["main.0.sin_inc"]).reshape(4, 4)
    return MetaKernelConfig(in_channels=int(w1.shape[0]), ndf=int(torch.as_tensor(state["main.0.coov.weight"]).shape[0]),
                            n_layers=len(coovs) - 2, azi=float(math.asin(float(sa[0, 3]))), inc=float(math.asin(float(si[3, 0]))),
                            range_mean=range_mean, range_std=range_std)


# ---- host statements ---------------------------------------------------------------------------------------------------------------
class _Bf16Linear(torch.autograd.Function):
    """a (rows, K) @ w (N, K)^T whose three GEMMs see bf16-rounded operands, as the kernels': forward r(a) r(w)^T; input gradient
    r(dy) r(w); weight gradient r(dy)^T r(a)."""

    @staticmethod
    def forward(ctx, a, w):
        ctx.save_for_backward(a, w)
        return _bf16(a) @ _bf16(w).t()

    @staticmethod
    def backward(ctx, dy):
        a, w = ctx.saved_tensors
        r = _bf16(dy)
        return r @ _bf16(w), r.t() @ _bf16(a)


def source_indices(W, H, stride):
    """-> (w_idx (Wo, 4) over j, h_idx (Ho, 4) over i, h_ok (Ho, 4)): the source column (wrapped) and row of every tap, and whether the
    row is inside [0, H)."""
    Wo, Ho = (W - 2) // stride + 1, (H - 2) // stride + 1
    w_idx = (stride * torch.arange(Wo)[:, None] + torch.arange(4)[None, :] - 1) % W
    h_idx = stride * torch.arange(Ho)[:, None] + torch.arange(4)[None, :] - 1
    return w_idx, h_idx, (h_idx >= 0) & (h_idx < H)


def _patches(t, stride, outside):
    """t (B, C, W, H) -> (B, Wo, Ho, 4 (i), 4 (j), C): the 4 x 4 window of every output pixel, W wrapped, `outside` beyond H."""
    W, H = t.shape[2:]
    w_idx, h_idx, h_ok = source_indices(W, H, stride)
    p = t[:, :, w_idx[:, None, None, :], h_idx.clamp(0, H - 1)[None, :, :, None]]              # (B, C, Wo, Ho, i, j)
    p = torch.where(h_ok[None, None, None, :, :, None], p, torch.as_tensor(outside, dtype=t.dtype))
    return p.permute(0, 2, 3, 4, 5, 1)


def _tables(state, name, dtype):
    return [torch.as_tensor(state[f"{name}.{t}"]).to(dtype).reshape(4, 4) for t in TABLES]


def _layer_torch(x, r, tabs, w1, b1, w2, b2, coov, bias, stride, bf16):
    """One layer in torch ops (differentiable): -> (out (B, N, Wo, Ho), r_c (B, 1, Wo, Ho))."""
    ca, sa, ci, si = tabs
    Cc, N = x.shape[1], coov.shape[0]
    rp = _patches(r, stride, R_OUTSIDE)[..., 0]                                                # (B, Wo, Ho, 4, 4)
    rc = rp[:, :, :, 2, 2]
    a = rp * ca
    pe = torch.stack([a * ci - rc[..., None, None], a * si, rp * sa], -1)                       # (B, Wo, Ho, 4, 4, 3)
    hid = F.leaky_relu(F.linear(pe, w1, b1), SLOPE)
    big = bf16 and Cc >= 16                                     # (the C = 2 layer's MLP runs in fp32 on the VALU)
    m = (_Bf16Linear.apply(hid.reshape(-1, Cc), w2).reshape(hid.shape) + b2) if big else F.linear(hid, w2, b2)
    P = (m * _patches(x, stride, 0.0)).reshape(-1, 16 * Cc)                                   # [(b, wo, ho)][t C + c]
    wc = coov.reshape(N, Cc, 16).permute(0, 2, 1).reshape(N, 16 * Cc)                         # [n][t C + c]
    y = (_Bf16Linear.apply(P, wc) if bf16 else P @ wc.t()) + bias
    B, Wo, Ho = rp.shape[:3]
    return y.reshape(B, Wo, Ho, N).permute(0, 3, 1, 2), rc[:, None]


def forward_host(state, x, training=True, bf16=False, buffers=None, detach_r=False, range_mean=20.0, range_std=40.0):
    """The network in plain torch: x (B, in_channels, W, H) -> logits (B, 1, Wo, Ho), differentiable in x (through the features AND
    through the range image: pe -> MLP -> m) and in every tensor of `state` that requires grad.  training, buffers: as
    discriminator.forward_host.  detach_r: the range path is cut (the tests' proof that it carries gradient).

    bf16: the operands of the kernels' four MFMA GEMMs are rounded to bf16 exactly where the kernels round them, everything else stays
    in x's dtype:
        m     = r(h) r(W2)^T + b2              input gradient r(dm) r(W2), weight gradient r(dm)^T r(h)      (layers with C >= 16 only:
                                               the C = 2 layer's MLP is fp32 throughout)
        out   = r(m x_patch) r(coov)^T + b     input gradient G = r(dy) r(coov), weight gradient r(dy)^T r(m x_patch)
    pe, the first Linear, LeakyReLU, the products m x_patch, G x_patch, G m, the first Linear's gradients, dr, the bias sums and m as
    it is kept for the backward are NOT rounded."""
    state = {k: torch.as_tensor(v) for k, v in state.items()}
    cfg = config_from_state(state, range_mean, range_std)
    if buffers is None:
        buffers = {k: v.detach().clone() for k, v in state.items() if k.endswith(BUFFER_SUFFIXES)}
    h = x
    r = (x[:, :1] * cfg.range_std + cfg.range_mean) / 10
    if detach_r:
        r = r.detach()
    for L in layer_specs(cfg):
        n = L["name"]
        g = lambda k: state[f"{n}.{k}"].to(h.dtype)             # noqa: E731
        h, r = _layer_torch(h, r, _tables(state, n, h.dtype), g("mlp_coord.0.weight"), g("mlp_coord.0.bias"), g("mlp_coord.2.weight"),
                            g("mlp_coord.2.bias"), g("coov.weight"), g("coov.bias"), L["stride"], bf16)
        if L["bn"]:
            h = batchnorm_running_host(h, state, buffers, L["bn"], training)
        if L["act"]:
            h = F.leaky_relu(h, SLOPE)
    return h


def _row_geometry(B, W, H, stride):
    """Per row (b, wo, ho, i, j) flattened: the source pixel index into (B, W, H) flattened (-1 outside H) and the centre's."""
    w_idx, h_idx, h_ok = source_indices(W, H, stride)
    Wo, Ho = w_idx.shape[0], h_idx.shape[0]
    b = torch.arange(B)[:, None, None, None, None]
    src = (b * W + w_idx[None, :, None, None, :]) * H + h_idx[None, None, :, :, None]
    src = torch.where(h_ok[None, None, :, :, None].expand_as(src), src, torch.full_like(src, -1))
    centre = src[:, :, :, 2, 2]
    return src.reshape(-1), centre.reshape(-1), Wo, Ho


def pe_host(r, tables, stride, dpe=None, dr_next=None):
    """rldm_train_meta's positional encoding (mk_pe_kernel / mk_dr_kernel) in fp64.  r (B, W, H); tables (4, 16) = cos_azi | sin_azi |
    cos_inc | sin_inc.  -> dict: pe (rows, 3), src (rows,), r_next (B, Wo, Ho) and, given dpe (rows, 3): dr (B, W, H), to which
    dr_next (B, Wo, Ho) is added at the centres."""
    r = torch.as_tensor(np.asarray(r), dtype=torch.float64)
    tab = torch.as_tensor(np.asarray(tables), dtype=torch.float64).reshape(4, 16)
    B, W, H = r.shape
    src, centre, Wo, Ho = _row_geometry(B, W, H, stride)
    rf = r.reshape(-1)
    inside = src >= 0
    rt = torch.where(inside, rf[src.clamp(min=0)], torch.tensor(R_OUTSIDE, dtype=torch.float64))
    rc = rf[centre]
    t = torch.arange(src.numel()) % 16
    ca, sa, ci, si = tab[0][t], tab[1][t], tab[2][t], tab[3][t]
    rc_rows = rc.repeat_interleave(16)
    pe = torch.stack([(rt * ca) * ci - rc_rows, (rt * ca) * si, rt * sa], 1)
    out = dict(pe=pe.numpy(), src=src.numpy().astype(np.int32), r_next=rc.reshape(B, Wo, Ho).numpy())
    if dpe is not None:
        d = torch.as_tensor(np.asarray(dpe), dtype=torch.float64).reshape(-1, 3)
        tap = (d[:, 0] * ci) * ca + (d[:, 1] * si) * ca + d[:, 2] * sa
        dr = torch.zeros(B * W * H, dtype=torch.float64)
        dr.index_add_(0, src[inside], tap[inside])
        cen = -d[:, 0].reshape(-1, 16).sum(1)
        if dr_next is not None:
            cen = cen + torch.as_tensor(np.asarray(dr_next), dtype=torch.float64).reshape(-1)
        dr.index_add_(0, centre, cen)
        out["dr"] = dr.reshape(B, W, H).numpy()
    return out


def mlp_host(pe, w1, b1, w2, b2, dm=None):
    """The modulation MLP in fp64: pe (rows, 3) -> m (rows, C) = W2 lrelu(W1 pe + b1) + b2 and, given dm: dw1, db1, dw2, db2, dpe.
    LeakyReLU's gradient at 0 is the slope-0.2 side."""
    f = lambda a: np.asarray(a, np.float64)                     # noqa: E731
    pe, w1, b1, w2, b2 = f(pe), f(w1), f(b1), f(w2), f(b2)
    pre = pe @ w1.T + b1
    h = np.where(pre > 0, pre, SLOPE * pre)
    out = dict(h=h, m=h @ w2.T + b2)
    if dm is not None:
        dm = f(dm)
        dpre = (dm @ w2) * np.where(pre > 0, 1.0, SLOPE)
        out.update(dw2=dm.T @ h, db2=dm.sum(0), dw1=dpre.T @ pe, db1=dpre.sum(0), dpe=dpre @ w1)
    return out


def modconv_host(x, src, m, coov, bias, dy=None):
    """The modulated 1 x 1 convolution over the 16 C tap-channels in fp64.  x (B, W, H, C) NHWC; src (rows,) from pe_host; m (rows, C);
    coov (N, 16 C) in the reference's order [c 16 + t].  -> dict: y (pixels, N) and, given dy (pixels, N): dx (B, W, H, C), dm
    (rows, C), dcoov (N, 16 C), dbias."""
    f = lambda a: np.asarray(a, np.float64)                     # noqa: E731
    x, m, coov, bias, src = f(x), f(m), f(coov), f(bias), np.asarray(src)
    Cc, N = x.shape[-1], coov.shape[0]
    xf = x.reshape(-1, Cc)
    xp = np.where((src >= 0)[:, None], xf[np.maximum(src, 0)], 0.0)                             # (rows, C)
    P = (m * xp).reshape(-1, 16 * Cc)                                                         # [px][t C + c]
    wc = coov.reshape(N, Cc, 16).transpose(0, 2, 1).reshape(N, 16 * Cc)
    out = dict(y=P @ wc.T + bias)
    if dy is not None:
        dy = f(dy).reshape(-1, N)
        G = (dy @ wc).reshape(-1, Cc)
        dx = np.zeros_like(xf)
        np.add.at(dx, src[src >= 0], (G * m)[src >= 0])
        out.update(dx=dx.reshape(x.shape), dm=G * xp, dbias=dy.sum(0),
                   dcoov=(dy.T @ P).reshape(N, 16, Cc).transpose(0, 2, 1).reshape(N, 16 * Cc))
    return out


def layer_host(x, r, tables, w1, b1, w2, b2, coov, bias, stride, dy=None, dr_next=None):
    """rldm_train_meta_forward / _backward in fp64 from the three statements above.  x (B, W, H, C), r (B, W, H) -> dict: y (B, Wo,
    Ho, N), r_next, pe, src, m and, given dy: dx, dr, dw1, db1, dw2, db2, dcoov, dbias."""
    x = np.asarray(x, np.float64)
    coov = np.asarray(coov, np.float64).reshape(np.asarray(coov).shape[0], -1)
    g = pe_host(r, tables, stride)
    mm = mlp_host(g["pe"], w1, b1, w2, b2)
    cv = modconv_host(x, g["src"], mm["m"], coov, bias, dy)
    B, Wo, Ho = g["r_next"].shape
    out = dict(y=cv["y"].reshape(B, Wo, Ho, -1), r_next=g["r_next"], pe=g["pe"], src=g["src"], m=mm["m"])
    if dy is not None:
        mb = mlp_host(g["pe"], w1, b1, w2, b2, cv["dm"])
        out.update(dx=cv["dx"], dcoov=cv["dcoov"], dbias=cv["dbias"], dw1=mb["dw1"], db1=mb["db1"], dw2=mb["dw2"], db2=mb["db2"],
                   dr=pe_host(r, tables, stride, mb["dpe"], dr_next)["dr"])
    return out


# ---- the kernels (device fp32, NHWC) ---------------------------------------------------------------------------------------------
def layer_desc(x_shape, N, stride):
    """The desc of a layer over an input (B, W, H, C); ValueError where the library has no instance."""
    d = _lib.TrainMetaDescC()
    d.B, d.Win, d.Hin, d.C = (int(v) for v in x_shape)
    d.N, d.stride = int(N), int(stride)
    if not _lib.lib().rldm_train_meta_ok(C.byref(d)):
        raise ValueError(f"no Meta-Kernel layer instance for input {tuple(x_shape)} (NHWC), N = {N}, stride {stride}: C is 2 or a "
                         f"multiple of 16, N is 1 or a multiple of 16, stride 1 or 2, extents >= 2")
    return d


def input_range(x, range_mean=20.0, range_std=40.0):
    """x (B, W, H, C) -> r (B, W, H) = (x[..., 0] range_std + range_mean) / 10."""
    r = T.empty(tuple(x.shape[:3]), x)
    _lib.check(_lib.lib().rldm_train_meta_range(_p(x), r.numel(), x.shape[3], float(range_mean), float(range_std), _p(r), _s(x)),
               "rldm_train_meta_range")
    return r


def input_range_backward(dr, dx, range_std=40.0):
    """dx[..., 0] += (dr / 10) range_std, in place."""
    _lib.check(_lib.lib().rldm_train_meta_range_grad(_p(dr), dr.numel(), dx.shape[3], float(range_std), _p(dx), _s(dx)),
               "rldm_train_meta_range_grad")
    return dx


def _ws(d, like):
    return _workspace(_lib.lib().rldm_train_meta_workspace(C.byref(d)), like)


def meta_forward(x, r, tables, w1, b1, w2, b2, coov, bias, stride):
    """x (B, W, H, C), r (B, W, H), tables (4, 16) -> (y (B, Wo, Ho, N), r_next (B, Wo, Ho), saved = (pe, src, m))."""
    N = coov.shape[0]
    d = layer_desc(x.shape, N, stride)
    B, W, H, Cc = x.shape
    Wo, Ho = D.conv_out_size(W, H, stride)
    rows = B * Wo * Ho * 16
    y, rn = T.empty((B, Wo, Ho, N), x), T.empty((B, Wo, Ho), x)
    pe, m = T.empty((rows, 3), x), T.empty((rows, Cc), x)
    src = torch.empty((rows,), dtype=torch.int32, device=x.device)
    ws = _ws(d, x)
    _lib.check(_lib.lib().rldm_train_meta_forward(C.byref(d), _p(x), _p(r), _p(tables), _p(w1), _p(b1), _p(w2), _p(b2), _p(coov), _p(bias),
                                                  _p(y), _p(rn), _p(pe), _p(src), _p(m), _p(ws), ws.numel(), _s(x)),
               "rldm_train_meta_forward")
    return y, rn, (pe, src, m)


def meta_backward(x, dy, tables, w1, b1, w2, coov, saved, stride, grads=None, want_input=True, want_range=True, dr_next=None):
    """grads: (dw1, db1, dw2, db2, dcoov, dbias) views into zeroed (or accumulating) gradient buffers, or None for the input gradient
    alone.  -> (dx, dr); dx is None without want_input, dr None without want_range (which needs want_input).  dr_next: the next layer's dr (B, Wo, Ho), added at the centres."""
    d = layer_desc(x.shape, coov.shape[0], stride)
    pe, src, m = saved
    dx = torch.empty_like(x) if want_input else None
    dr = T.empty(tuple(x.shape[:3]), x) if want_input and want_range else None
    g = grads if grads is not None else (None,) * 6
    ws = _ws(d, x)
    _lib.check(_lib.lib().rldm_train_meta_backward(C.byref(d), _p(x), _p(dy), _p(tables), _p(w1), _p(b1), _p(w2), _p(coov), _p(pe), _p(src),
                                                   _p(m), _p(dr_next), _p(dx), _p(dr), *[_p(t) for t in g], _p(ws), ws.numel(), _s(x)),
               "rldm_train_meta_backward")
    return dx, dr


# ---- the network on the tape -------------------------------------------------------------------------------------------------------
LAYER_PARAMS = (".mlp_coord.0.weight", ".mlp_coord.0.bias", ".mlp_coord.2.weight", ".mlp_coord.2.bias", ".coov.weight", ".coov.bias")


class MetaKernelDiscriminator(PatchDiscriminator):
    """PatchDiscriminator with the Meta-Kernel layer in place of the conv.  The walk over the layers with its BatchNorm / LeakyReLU
    tail, the losses, the optimizer step and the state handling are PatchDiscriminator's, unchanged; this class states the layer
    (`_layer_forward` / `_layer_backward`: rldm_train_meta_* with the range image threaded from layer to layer on the pass, the input's
    range mapping in front of the first layer and its gradient behind it) and keeps the tables: buffers of the state, handed to
    the kernels as one (4, 16) argument per layer.  The kernels read the fp32 masters, so no weight has a bf16 operand copy."""

    def __init__(self, config=None, state=None, seed=0, device="cuda", lr=4.5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 deterministic=False):
        cfg = _cfg(config) if state is None or config is not None else config_from_state(state)
        state = state if state is not None else init_state(cfg, seed)
        self._build(cfg, state, layer_specs(cfg), param_shapes(cfg), trainable_names(cfg), BUFFER_SUFFIXES + TABLE_SUFFIXES, device,
                    dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=None), deterministic, packed=())
        self.tables = {L["name"]: self._table(L["name"]).contiguous() for L in self.specs}

    def _table(self, n):
        return torch.cat([self.buffers[f"{n}.{t}"].reshape(1, 16) for t in TABLES])

    def _layer_forward(self, ps, L, x):
        n = L["name"]
        if L is self.specs[0]:
            ps.r = input_range(x, self.cfg.range_mean, self.cfg.range_std)
        y, ps.r, saved = meta_forward(x, ps.r, self.tables[n], *[self.p[n + k] for k in LAYER_PARAMS], L["stride"])
        return y, saved

    def _layer_backward(self, ps, L, x, dy, saved, params, want_input):
        """As PatchDiscriminator's; ps.dr carries the range image's gradient from the layer behind to the layer in front.  The range
        path ends at the input: without want_input no layer computes dr."""
        n = L["name"]
        first, last = L is self.specs[0], L is self.specs[-1]
        w1, b1, w2, _, coov, _ = [self.p[n + k] for k in LAYER_PARAMS]
        dx, ps.dr = meta_backward(x, dy, self.tables[n], w1, b1, w2, coov, saved, L["stride"],
                                  [self.g[n + k] for k in LAYER_PARAMS] if params else None, want_input=want_input or not first,
                                  want_range=want_input, dr_next=None if last else ps.dr)
        return input_range_backward(ps.dr, dx, self.cfg.range_std) if first and want_input else dx

    def load_payload(self, st):
        super().load_payload(st)
        for n, t in self.tables.items():
            t.copy_(self._table(n))


