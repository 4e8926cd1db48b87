#!/usr/bin/env python3
"""CPU: how large is the gradient error that bf16 conv operands ALONE cause in the VAE -- its decoder, and the whole step?

    python tools/vae_bf16_floor.py

The training convs round x, w and dy to bf16 and accumulate in fp32; everything else on the tape is fp32.  This runs the oracle
(oracle/vae.py) twice on the host -- plain fp32 autograd, and with every conv's operands rounded to bf16 in forward, data gradient and
weight gradient -- and prints the relative L2 distance of the prediction, of the flat gradient buffer and of the worst parameter:
the decoder on the two configurations and inputs of tests/test_vae_training_gpu.py, then encoder + posterior + decoder with
loss = L1 + kl_weight * kl on those of tests/test_vae_encoder_training_gpu.py (the L1 target planted around the fp32 prediction in
both runs).  It is the floor the device's gradient errors sit on, and what those tests' gates are read against."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ops as o_ops  # noqa: E402
from oracle import vae as o_vae  # noqa: E402
from rangeldm_amd.config import VAEConfig  # noqa: E402
from rangeldm_amd.params import vae_param_shapes  # noqa: E402
from rangeldm_amd.synth import synth_state_dict  # noqa: E402

fp32_conv = o_ops.circ_conv2d
fp32_down = o_ops.downsample_vae


def bf16(t):
    return t.to(torch.bfloat16).float()


class Bf16OperandConv(torch.autograd.Function):
    """circ_conv2d with x, w (forward), dy, w (data gradient) and dy, x (weight gradient) rounded to bf16; fp32 accumulation."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.geometry = (stride, padding)
        return fp32_conv(bf16(x), bf16(w), b, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, padding = ctx.geometry
        with torch.enable_grad():
            xr, wr = bf16(x).requires_grad_(), bf16(w).requires_grad_()
            dx, dw = torch.autograd.grad(fp32_conv(xr, wr, None, stride, padding), [xr, wr], bf16(dy))
        return dx, dw, dy.sum((0, 2, 3)), None, None


class Bf16OperandDown(torch.autograd.Function):
    """downsample_vae (the encoder's end-padded stride-2 conv) with the same roundings."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return fp32_down(bf16(x), bf16(w), b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            xr, wr = bf16(x).requires_grad_(), bf16(w).requires_grad_()
            dx, dw = torch.autograd.grad(fp32_down(xr, wr, None), [xr, wr], bf16(dy))
        return dx, dw, dy.sum((0, 2, 3))


def _round_convs(rounded):
    o_ops.circ_conv2d = (lambda x, w, b, stride=1, padding=1: Bf16OperandConv.apply(x, w, b, stride, padding)) if rounded else fp32_conv
    o_ops.downsample_vae = Bf16OperandDown.apply if rounded else fp32_down


def whole_step(cfg, B, rounded, kl_weights, target=None):
    """tests/test_vae_encoder_training_gpu.py::oracle_step -> (moments, prediction, target, {kl_weight: gradients})."""
    _round_convs(rounded)
    try:
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(17)
        f = cfg.downscale
        images = torch.rand(B, cfg.in_channels, *cfg.sample_size, generator=g)
        noise = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        sdt = {k: torch.from_numpy(np.array(v)).float().requires_grad_() for k, v in sd.items()}
        moments = o_vae.vae_encode.__wrapped__(sdt, cfg, images)
        d = o_vae.DiagonalGaussian(moments)
        pred = o_vae.vae_decode.__wrapped__(sdt, cfg, d.sample(noise=noise))
        if target is None:
            s = torch.randint(0, 2, pred.shape, generator=g).float() * 2 - 1
            target = (pred.detach() + s * (0.25 + 0.25 * torch.rand(pred.shape, generator=g))).contiguous()
        rec = (torch.tensor((40.0, 10.0))[None, :, None, None] * (pred - target).abs()).sum() / B
        kl = 0.5 * (d.mean ** 2 + torch.exp(d.logvar) - 1 - d.logvar).sum() / B
        keys = list(sdt)
        grads = {kw: dict(zip(keys, torch.autograd.grad(rec + kw * kl, [sdt[k] for k in keys], retain_graph=True))) for kw in kl_weights}
        return moments.detach(), pred.detach(), target, grads
    finally:
        _round_convs(False)


def compare(g0, g1):
    """-> (error over the flat buffer, (worst per-parameter error, its name)): the measure of the tests' _gradient_errors."""
    f0 = torch.cat([g0[k].reshape(-1) for k in g0]).double()
    f1 = torch.cat([g1[k].reshape(-1) for k in g0]).double()
    rms = float(f0.norm() / f0.numel() ** 0.5)
    worst = max((float((g1[k].double() - g0[k].double()).norm()) / (float(g0[k].double().norm()) + 2e-2 * rms * g0[k].numel() ** 0.5), k)
                for k in g0)
    return float((f1 - f0).norm() / f0.norm()), worst


def gradients(cfg, B, rounded):
    _round_convs(rounded)
    try:
        sd = synth_state_dict(vae_param_shapes(cfg), prefix="vt.")
        g = torch.Generator().manual_seed(7)
        f = cfg.downscale
        z = torch.randn(B, cfg.z_channels, cfg.sample_size[0] // f, cfg.sample_size[1] // f, generator=g)
        dpred = torch.randn(B, cfg.out_channels, *cfg.sample_size, generator=g)
        keys = [k for k in sd if k.startswith("decoder.")]
        sdt = {k: torch.from_numpy(np.array(sd[k])).float().requires_grad_() for k in keys}
        pred = o_vae.vae_decode.__wrapped__(sdt, cfg, z)
        return pred.detach(), dict(zip(keys, torch.autograd.grad(pred, [sdt[k] for k in keys], grad_outputs=dpred)))
    finally:
        _round_convs(False)


def main():
    for name, cfg, B in (("SMALL", VAEConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, sample_size=(32, 8)), 3),
                         ("TALL", VAEConfig(ch=64, ch_mult=(1, 2, 4), num_res_blocks=2, sample_size=(32, 64)), 2)):
        p0, g0 = gradients(cfg, B, False)
        p1, g1 = gradients(cfg, B, True)
        err_all, worst = compare(g0, g1)
        print(f"{name}: forward {float((p1 - p0).double().norm() / p0.double().norm()):.3g}, all parameters "
              f"{err_all:.3g}, worst parameter {worst[0]:.3g} ({worst[1]})")
        kws = (1e-6, 1.0) if name == "SMALL" else (1e-6,)
        m0, p0, target, g0 = whole_step(cfg, B, False, kws)
        m1, p1, _, g1 = whole_step(cfg, B, True, kws, target)
        for kw in kws:
            err_all, worst = compare(g0[kw], g1[kw])
            print(f"{name} encoder + decoder, kl_weight {kw:g}: moments {float((m1 - m0).double().norm() / m0.double().norm()):.3g}, "
                  f"forward {float((p1 - p0).double().norm() / p0.double().norm()):.3g}, all parameters {err_all:.3g}, "
                  f"worst parameter {worst[0]:.3g} ({worst[1]})")


if __name__ == "__main__":
    main()
