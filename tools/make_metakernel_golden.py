#!/usr/bin/env python3
"""Write tests/golden/metakernel.npz: what the reference's Meta-Kernel discriminator computes, recorded on CPU fp32.

    python tools/make_metakernel_golden.py --reference /path/to/RangeLDM [--out tests/golden/metakernel.npz]

The reference's own code does the computing: `NLayerDiscriminatorMetaKernel` (vae/sgm/modules/autoencoding/lpips/model/model.py) and
`hinge_d_loss` (lpips/vqperceptual.py) are loaded by file path, with tools/make_discriminator_golden.py's stub in place of
lpips/util.py (use_actnorm stays False).  The state is rangeldm_amd.metakernel.init_state(cfg, SEED), loaded with strict=True -- the
four tables of every layer included, so the module computes with this project's tables, which the file also records next to the ones
the reference's constructor built --; the module stays in training mode, as in both of the reference's uses.  Only arrays are written.

One case per (ndf, size): B = 2, ndf in (16, 64), inputs (2, 2, 32, 24) and (2, 2, 64, 32); 24 beams are the fewest that leave a
logit.  The sequence is the reference's discriminator step followed by its generator term on the same fake pass: forward(real),
forward(fake), d = hinge_d_loss(real logits, fake logits), g = -mean(fake logits).

Keys (case prefix `n{ndf}_{W}x{H}_`): as tests/golden/discriminator.npz's -- seed, keys, x{W}x{H}_real / _fake, logits_real / _fake,
d_loss, g_loss, d_grad.<key> / g_grad.<key> (the elements discriminator.grad_sample_indices(numel) of the flattened gradient; <key>
also `real`, `fake`), d_norm.<key> / g_norm.<key> (the L2 norm of the WHOLE gradient; for the inputs also `<key>.c0`, `<key>.c1`: the
norms of channel 0, which carries the range path, and channel 1), buf.<key>, threads_rel -- and `ref_table.<key>`: the tables the
reference's constructor built for ndf = 64 before the state was loaded; `null_grads`: the parameters whose gradient is zero in
exact arithmetic (null_gradients below).  Their recorded gradients are rounding noise (norms around 1e-7 where their neighbours'
are around 1e-1) and differ from run to run, so threads_rel leaves them out and a test can only bound them.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rangeldm_amd import discriminator as D             # noqa: E402
from rangeldm_amd import metakernel as MK               # noqa: E402
from make_discriminator_golden import load_reference    # noqa: E402

SEED = 7
SIZES = ((32, 24), (64, 32))
WIDTHS = (16, 64)


def null_gradients(ndf):
    """The parameters whose gradient is zero in exact arithmetic: a coov.bias in front of a BatchNorm (the batch mean takes it out
    again).  What autograd records for them is rounding noise, different from run to run."""
    return [L["name"] + ".coov.bias" for L in MK.layer_specs(MK.MetaKernelConfig(ndf=ndf)) if L["bn"]]


def run_case(Net, hinge_d_loss, ndf, real, fake):
    cfg = MK.MetaKernelConfig(in_channels=2, ndf=ndf, n_layers=3)
    net = Net(input_nc=2, ndf=ndf, n_layers=3, azi=cfg.azi, inc=cfg.inc, log=False, range_mean=cfg.range_mean, range_std=cfg.range_std)
    ref_tables = {k: v.numpy().copy() for k, v in net.state_dict().items() if k.endswith(MK.TABLE_SUFFIXES)}
    net.load_state_dict(MK.init_state(cfg, SEED), strict=True)
    net.train()
    real, fake = real.clone().requires_grad_(), fake.clone().requires_grad_()
    lr, lf = net(real), net(fake)
    d, g = hinge_d_loss(lr, lf), -torch.mean(lf)
    params = dict(net.named_parameters())
    wrt = list(params.values()) + [real, fake]
    names = list(params) + ["real", "fake"]
    out = {"logits_real": lr.detach().numpy(), "logits_fake": lf.detach().numpy(), "d_loss": np.float64(d.item()),
           "g_loss": np.float64(g.item())}
    for tag, loss in (("d", d), ("g", g)):
        grads = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)
        for n, gr in zip(names, grads):
            if gr is None:
                assert tag == "g" and n == "real"
                continue
            flat = gr.reshape(-1)
            out[f"{tag}_grad.{n}"] = flat[torch.from_numpy(D.grad_sample_indices(flat.numel()))].numpy()
            out[f"{tag}_norm.{n}"] = np.float64(flat.double().norm().item())
            if n in ("real", "fake"):
                for c in (0, 1):
                    out[f"{tag}_norm.{n}.c{c}"] = np.float64(gr[:, c].double().norm().item())
    for k, v in net.state_dict().items():
        if k.endswith(D.BUFFER_SUFFIXES):
            out["buf." + k] = v.numpy().copy()
    return out, list(net.state_dict().keys()), ref_tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "metakernel.npz"))
    a = ap.parse_args()
    NLayerDiscriminator, hinge_d_loss = load_reference(a.reference)
    Net = sys.modules["ref_lpips.model.model"].NLayerDiscriminatorMetaKernel
    out = {"seed": np.int64(SEED)}
    threads = torch.get_num_threads()
    for W, H in SIZES:
        g = torch.Generator().manual_seed(1000 + W)
        real, fake = torch.randn((2, 2, W, H), generator=g), torch.randn((2, 2, W, H), generator=g) * 0.8 + 0.1
        out[f"x{W}x{H}_real"], out[f"x{W}x{H}_fake"] = real.numpy(), fake.numpy()
        for ndf in WIDTHS:
            case, keys, ref_tables = run_case(Net, hinge_d_loss, ndf, real, fake)
            torch.set_num_threads(1)
            again, _, _ = run_case(Net, hinge_d_loss, ndf, real, fake)
            torch.set_num_threads(threads)
            rel = 0.0
            null = [f"{tag}_grad.{n}" for tag in "dg" for n in null_gradients(ndf)]
            for k, v in case.items():
                if k in null or k.replace("_norm.", "_grad.") in null:
                    continue
                v64, w64 = np.asarray(v, np.float64), np.asarray(again[k], np.float64)
                rel = max(rel, float(np.linalg.norm(v64 - w64) / (np.linalg.norm(v64) + 1e-300)))
            print(f"ndf {ndf} {W}x{H}: logits {case['logits_real'].shape}, d {case['d_loss']:.6f}, g {case['g_loss']:.6f}, "
                  f"{threads} threads against 1: rel-L2 {rel:.2e}")
            case["threads_rel"] = np.float64(rel)
            out.update({f"n{ndf}_{W}x{H}_{k}": v for k, v in case.items()})
            if ndf == 64:
                out["keys"] = np.array(keys)
                out["null_grads"] = np.array(null_gradients(ndf))
                out.update({"ref_table." + k: v for k, v in ref_tables.items()})
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
