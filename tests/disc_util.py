"""What tests/test_discriminator_host.py and tests/test_discriminator_gpu.py share: the golden file of the reference's PatchGAN
(tools/make_discriminator_golden.py) and the same sequence -- forward(real), forward(fake), hinge loss, generator term -- on
rangeldm_amd.discriminator.forward_host, computed once per (ndf, size, bf16) and left unchanged."""
import os

import numpy as np
import torch

from rangeldm_amd import discriminator as D

_GOLDEN = None
CASES = [(16, 32, 24), (64, 32, 24), (16, 64, 32), (64, 64, 32)]


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "discriminator.npz")) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


def golden_case(ndf, W, H):
    """The arrays of one case without their prefix, plus the two inputs as `real` / `fake`."""
    g, pre = golden(), f"n{ndf}_{W}x{H}_"
    out = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    out["real"], out["fake"] = g[f"x{W}x{H}_real"], g[f"x{W}x{H}_fake"]
    return out


def init(ndf):
    return D.init_state(D.DiscriminatorConfig(2, ndf, 3), int(golden()["seed"]))


_HOST = {}


def host_case(ndf, W, H, bf16=False):
    """forward_host's version of a golden case: logits, losses, buffers after the two passes, and the FULL gradients of d and g as
    `d_full.<key>` / `g_full.<key>` (torch tensors; keys as the golden's, `real` / `fake` for the inputs)."""
    key = (ndf, W, H, bf16)
    if key not in _HOST:
        gc = golden_case(ndf, W, H)
        state = init(ndf)
        names = D.trainable_names(D.config_from_state(state))
        for n in names:
            state[n].requires_grad_()
        buffers = {k: v.clone() for k, v in state.items() if k.endswith(D.BUFFER_SUFFIXES)}
        real, fake = torch.from_numpy(gc["real"]).clone().requires_grad_(), torch.from_numpy(gc["fake"]).clone().requires_grad_()
        lr = D.forward_host(state, real, True, bf16, buffers)
        lf = D.forward_host(state, fake, True, bf16, buffers)
        d, g = D.hinge_d_loss_host(lr, lf), -torch.mean(lf)
        out = {"logits_real": lr.detach(), "logits_fake": lf.detach(), "d_loss": float(d.detach()), "g_loss": float(g.detach())}
        wrt = [state[n] for n in names] + [real, fake]
        for tag, loss in (("d", d), ("g", g)):
            grads = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)
            for n, gr in zip(names + ["real", "fake"], grads):
                if gr is not None:
                    out[f"{tag}_full.{n}"] = gr.detach()
        out.update({"buf." + k: v for k, v in buffers.items()})
        _HOST[key] = out
    return _HOST[key]


def sampled(t):
    """The elements of a gradient that the golden records."""
    flat = torch.as_tensor(t).reshape(-1)
    return flat[torch.from_numpy(D.grad_sample_indices(flat.numel()))]


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))
