#!/usr/bin/env python3
"""CPU: how large is the gradient error that bf16 conv operands ALONE cause in the VAE decoder?

    python tools/vae_bf16_floor.py

The training convs round x, w and dy to bf16 and accumulate in fp32; everything else on the tape is fp32.  This runs the oracle's decoder
(oracle/vae.py) twice on the host -- plain fp32 autograd, and with every conv's operands rounded to bf16 in forward, data gradient and
weight gradient -- on the two configurations and inputs of tests/test_vae_training_gpu.py and prints the relative L2 distance of the
prediction, of the flat gradient buffer and of the worst parameter (that test's measure).  It is the floor the device's gradient errors
sit on, and where that test's gates come from."""
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


def gradients(cfg, B, rounded):
    o_ops.circ_conv2d = (lambda x, w, b, stride=1, padding=1: Bf16OperandConv.apply(x, w, b, stride, padding)) if rounded else fp32_conv
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
        o_ops.circ_conv2d = fp32_conv


def main():
    for name, cfg, B in (("SMALL", VAEConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, sample_size=(32, 8)), 3),
                         ("TALL", VAEConfig(ch=64, ch_mult=(1, 2, 4), num_res_blocks=2, sample_size=(32, 64)), 2)):
        p0, g0 = gradients(cfg, B, False)
        p1, g1 = gradients(cfg, B, True)
        f0 = torch.cat([g0[k].reshape(-1) for k in g0]).double()
        f1 = torch.cat([g1[k].reshape(-1) for k in g0]).double()
        rms = float(f0.norm() / f0.numel() ** 0.5)
        worst = max((float((g1[k].double() - g0[k].double()).norm()) / (float(g0[k].double().norm()) + 2e-2 * rms * g0[k].numel() ** 0.5), k)
                    for k in g0)
        print(f"{name}: forward {float((p1 - p0).double().norm() / p0.double().norm()):.3g}, all parameters "
              f"{float((f1 - f0).norm() / f0.norm()):.3g}, worst parameter {worst[0]:.3g} ({worst[1]})")


if __name__ == "__main__":
    main()
