#!/usr/bin/env python3
"""Write tests/golden/discriminator.npz: what the reference's PatchGAN computes, recorded on CPU fp32.

    python tools/make_discriminator_golden.py --reference /path/to/RangeLDM [--out tests/golden/discriminator.npz]

The reference's own code does the computing: `NLayerDiscriminator` (vae/sgm/modules/autoencoding/lpips/model/model.py) and
`hinge_d_loss` (lpips/vqperceptual.py) are loaded by file path.  model.py imports `..util` for ActNorm, and that module imports
`requests` and `tqdm`; a stub module with an ActNorm placeholder is registered in its place (use_actnorm stays False).  The state is
rangeldm_amd.discriminator.init_state(cfg, SEED), loaded with strict=True; the module stays in training mode, as in both of the
reference's uses.  Only arrays are written.

One case per (ndf, size): B = 2, ndf in (16, 64), inputs (2, 2, 32, 24) and (2, 2, 64, 32); 24 beams are the fewest that leave a
logit (24 -> 12 -> 6 -> 3 -> 2 -> 1).  The sequence is the reference's discriminator step followed by its generator term on the same fake pass:
forward(real), forward(fake), d = hinge_d_loss(real logits, fake logits), g = -mean(fake logits).

Keys (case prefix `n{ndf}_{W}x{H}_`)
  seed, keys                          init_state's seed; the reference module's state_dict() keys for ndf = 64, in order
  x{W}x{H}_real / _fake               the inputs, shared by both widths
  logits_real, logits_fake            (2, 1, Wo, Ho)
  d_loss, g_loss                      float64 scalars (the fp32 results)
  d_grad.<key>, g_grad.<key>          autograd's gradient of d / g with respect to the parameter <key>: the elements
                                      discriminator.grad_sample_indices(numel) of the flattened gradient (all of a tensor up to 1 024
                                      elements, 1 024 evenly spaced ones of a larger one: the weights of ndf = 64 alone are 2.7 M values)
  d_norm.<key>, g_norm.<key>          the L2 norm of the WHOLE gradient, float64
  d_grad.real, d_grad.fake, g_grad.fake / _norm.*   the same for the gradients with respect to the inputs
  buf.<key>                           running_mean / running_var / num_batches_tracked after the two passes
  threads_rel                         the largest relative L2 distance between this run and the same run with one thread, over all
                                      arrays of the case (the reference's own reproducibility; tests/test_discriminator_host.py gates on
                                      max(this, 1e-5))
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rangeldm_amd import discriminator as D             # noqa: E402

LPIPS = "vae/sgm/modules/autoencoding/lpips"
SEED = 7
SIZES = ((32, 24), (64, 32))
WIDTHS = (16, 64)


def load_reference(root):
    """(NLayerDiscriminator, hinge_d_loss) from the reference's files, with a stub in place of lpips/util.py."""
    pkg = types.ModuleType("ref_lpips")
    pkg.__path__ = []
    sub = types.ModuleType("ref_lpips.model")
    sub.__path__ = []
    util = types.ModuleType("ref_lpips.util")
    util.ActNorm = type("ActNorm", (torch.nn.Module,), {})
    sys.modules.update({"ref_lpips": pkg, "ref_lpips.model": sub, "ref_lpips.util": util})
    spec = importlib.util.spec_from_file_location("ref_lpips.model.model", os.path.join(root, LPIPS, "model/model.py"))
    model = importlib.util.module_from_spec(spec)
    sys.modules["ref_lpips.model.model"] = model
    spec.loader.exec_module(model)
    spec = importlib.util.spec_from_file_location("ref_vqperceptual", os.path.join(root, LPIPS, "vqperceptual.py"))
    vq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vq)
    return model.NLayerDiscriminator, vq.hinge_d_loss


def run_case(NLayerDiscriminator, hinge_d_loss, ndf, real, fake):
    cfg = D.DiscriminatorConfig(in_channels=2, ndf=ndf, n_layers=3)
    net = NLayerDiscriminator(input_nc=2, ndf=ndf, n_layers=3)
    net.load_state_dict(D.init_state(cfg, SEED), strict=True)
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
    for k, v in net.state_dict().items():
        if k.endswith(D.BUFFER_SUFFIXES):
            out["buf." + k] = v.numpy().copy()
    return out, list(net.state_dict().keys())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "discriminator.npz"))
    a = ap.parse_args()
    NLayerDiscriminator, hinge_d_loss = load_reference(a.reference)
    out = {"seed": np.int64(SEED)}
    threads = torch.get_num_threads()
    for W, H in SIZES:
        g = torch.Generator().manual_seed(1000 + W)
        real, fake = torch.randn((2, 2, W, H), generator=g), torch.randn((2, 2, W, H), generator=g) * 0.8 + 0.1
        out[f"x{W}x{H}_real"], out[f"x{W}x{H}_fake"] = real.numpy(), fake.numpy()
        for ndf in WIDTHS:
            case, keys = run_case(NLayerDiscriminator, hinge_d_loss, ndf, real, fake)
            torch.set_num_threads(1)
            again, _ = run_case(NLayerDiscriminator, hinge_d_loss, ndf, real, fake)
            torch.set_num_threads(threads)
            rel = 0.0
            for k, v in case.items():
                v64, w64 = np.asarray(v, np.float64), np.asarray(again[k], np.float64)
                rel = max(rel, float(np.linalg.norm(v64 - w64) / (np.linalg.norm(v64) + 1e-300)))
            print(f"ndf {ndf} {W}x{H}: logits {case['logits_real'].shape}, d {case['d_loss']:.6f}, g {case['g_loss']:.6f}, "
                  f"{threads} threads against 1: rel-L2 {rel:.2e}")
            case["threads_rel"] = np.float64(rel)
            out.update({f"n{ndf}_{W}x{H}_{k}": v for k, v in case.items()})
            if ndf == 64:
                out["keys"] = np.array(keys)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
