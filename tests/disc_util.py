"""What the host and GPU tests of the two discriminators share: the golden file of the reference's network
(tools/make_discriminator_golden.py, tools/make_metakernel_golden.py), the same sequence -- forward(real), forward(fake), hinge loss,
generator term -- on the module's forward_host, computed once per (ndf, size, bf16, detach_r) and left unchanged, the same sequence
on the device with its figures (network_figures), and the two behaviour tests that are one text over two classes.  `PATCH`
(rangeldm_amd.discriminator, PatchDiscriminator) and `META` (rangeldm_amd.metakernel, MetaKernelDiscriminator) are the two families;
a test file takes one of them as `U`."""
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import discriminator as D
from rangeldm_amd import metakernel as MK


def sampled(t):
    """The elements of a gradient that the golden records."""
    flat = torch.as_tensor(t).reshape(-1)
    return flat[torch.from_numpy(D.grad_sample_indices(flat.numel()))]


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


class mode:
    """The library's deterministic switch for the duration of a block."""

    def __init__(self, det):
        self.det = det

    def __enter__(self):
        from rangeldm_amd import train_ops as T
        self.prev = T.deterministic_enabled()
        T.deterministic(self.det)

    def __exit__(self, *exc):
        from rangeldm_amd import train_ops as T
        T.deterministic(self.prev)


def param_errors(got, ref, names):
    """(worst per-parameter relative L2 with the floor of tests/test_training.py, its name, relative L2 over the flat buffer)."""
    flat_ref = torch.cat([ref[n].reshape(-1).double() for n in names])
    flat_got = torch.cat([got[n].reshape(-1).double().cpu() for n in names])
    rms = float(flat_ref.norm() / flat_ref.numel() ** 0.5)

    def err(n):
        d = float((got[n].double().cpu() - ref[n].double()).norm())
        return d / (float(ref[n].double().norm()) + 2e-2 * rms * ref[n].numel() ** 0.5)
    worst = max((err(n), n) for n in names)
    return worst[0], worst[1], float((flat_got - flat_ref).norm() / flat_ref.norm())


class Family:
    """One discriminator: its module (layer_specs, init_state, forward_host ... under the same names in both), its golden file,
    its config and network classes, and the top-level keys of the state file it writes."""
    CASES = [(16, 32, 24), (64, 32, 24), (16, 64, 32), (64, 64, 32)]
    STATE_KEYS = {"params", "exp_avg", "exp_avg_sq", "global_step", "names", "buffers"}
    rel, sampled = staticmethod(rel), staticmethod(sampled)

    def __init__(self, module, golden_file, config, network):
        self.module, self.golden_file, self.config, self.network = module, golden_file, config, network
        self._golden, self._host = None, {}

    def golden(self):
        if self._golden is None:
            with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", self.golden_file)) as z:
                self._golden = {k: z[k] for k in z.files}
        return self._golden

    def golden_case(self, ndf, W, H):
        """The arrays of one case without their prefix, plus the two inputs as `real` / `fake`."""
        g, pre = self.golden(), f"n{ndf}_{W}x{H}_"
        out = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
        out["real"], out["fake"] = g[f"x{W}x{H}_real"], g[f"x{W}x{H}_fake"]
        return out

    def init(self, ndf):
        return self.module.init_state(self.config(2, ndf, 3), int(self.golden()["seed"]))

    def host_case(self, ndf, W, H, bf16=False, **kw):
        """forward_host's version of a golden case: logits, losses, buffers after the two passes, and the FULL gradients of d and g as
        `d_full.<key>` / `g_full.<key>` (torch tensors; keys as the golden's, `real` / `fake` for the inputs).  kw: passed through to
        forward_host (the Meta-Kernel's detach_r)."""
        M = self.module
        key = (ndf, W, H, bf16, tuple(sorted(kw.items())))
        if key not in self._host:
            gc = self.golden_case(ndf, W, H)
            state = self.init(ndf)
            names = M.trainable_names(M.config_from_state(state))
            for n in names:
                state[n].requires_grad_()
            buffers = {k: v.clone() for k, v in state.items() if k.endswith(D.BUFFER_SUFFIXES)}
            real, fake = torch.from_numpy(gc["real"]).clone().requires_grad_(), torch.from_numpy(gc["fake"]).clone().requires_grad_()
            lr = M.forward_host(state, real, True, bf16, buffers, **kw)
            lf = M.forward_host(state, fake, True, bf16, buffers, **kw)
            d, g = D.hinge_d_loss_host(lr, lf), -torch.mean(lf)
            out = {"logits_real": lr.detach(), "logits_fake": lf.detach(), "d_loss": float(d.detach()), "g_loss": float(g.detach())}
            wrt = [state[n] for n in names] + [real, fake]
            for tag, loss in (("d", d), ("g", g)):
                grads = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)
                for n, gr in zip(names + ["real", "fake"], grads):
                    if gr is not None:
                        out[f"{tag}_full.{n}"] = gr.detach()
            out.update({"buf." + k: v for k, v in buffers.items()})
            self._host[key] = out
        return self._host[key]

    # ---- on the device ---------------------------------------------------------------------------------------------------------------
    def network_figures(self, ndf, W, H, dx_figures, det=False):
        """One run of the golden's sequence on the device -> (the device's figures, forward_host(bf16=True)'s): each figure is a
        distance from the reference's recording (through forward_host in fp32, which the host tests tie to the golden arrays).
        dx_figures(tag, got, ref) -> {figure name: value} for the input gradients (`got`, `ref`: dicts with `real` / `fake`)."""
        gc, hc, he = self.golden_case(ndf, W, H), self.host_case(ndf, W, H), self.host_case(ndf, W, H, bf16=True)
        disc = self.network(state=self.init(ndf), deterministic=det)
        names = disc.names
        real, fake = torch.from_numpy(gc["real"]).cuda(), torch.from_numpy(gc["fake"]).cuda()
        with mode(det):
            lr_ = disc.forward(real)
            pr, logits_real = disc._pass, disc.logits().cpu()
            lf = disc.forward(fake)
            pf, logits_fake = disc._pass, disc.logits().cpu()
            out, dreal, dfake = D.hinge(lr_, lf, 1.0)
            disc._backward(pr, dreal, True, False)
            disc._backward(pf, dfake, True, False)
            d_grads = {n: disc.g[n].cpu().clone() for n in names}
            d_grads["real"], d_grads["fake"] = nchw(disc._backward(pr, dreal, False, True)), nchw(disc._backward(pf, dfake, False, True))
            assert torch.equal(torch.cat([d_grads[n].reshape(-1) for n in names]), disc.grads.cpu())      # the input gradient touched no parameter
            disc.grads.zero_()
            g, dlog = disc.generator_loss()
            disc.backward(dlog)
            g_grads = {n: disc.g[n].cpu().clone() for n in names}
            g_grads["fake"] = nchw(disc.input_gradient(dlog))
        sd = disc.state_dict()
        if ndf == 64:
            assert list(sd) == [str(k) for k in self.golden()["keys"]]
        fig, floor = {}, {}
        for dst, src in ((fig, dict(logits_real=logits_real, logits_fake=logits_fake, d_loss=float(out[0]), g_loss=float(g), d=d_grads, g=g_grads,
                                    buf={k: sd[k] for k in sd if k.endswith(D.BUFFER_SUFFIXES)})),
                         (floor, dict(logits_real=he["logits_real"], logits_fake=he["logits_fake"], d_loss=he["d_loss"], g_loss=he["g_loss"],
                                      d={k[7:]: v for k, v in he.items() if k.startswith("d_full.")},
                                      g={k[7:]: v for k, v in he.items() if k.startswith("g_full.")},
                                      buf={k[4:]: v for k, v in he.items() if k.startswith("buf.")}))):
            dst["logits"] = max(rel(src["logits_real"], gc["logits_real"]), rel(src["logits_fake"], gc["logits_fake"]))
            dst["d_loss"] = abs(src["d_loss"] - float(gc["d_loss"])) / abs(float(gc["d_loss"]))
            dst["g_loss"] = abs(src["g_loss"] - float(gc["g_loss"])) / abs(float(gc["g_loss"]))
            for tag in ("d", "g"):
                ref = {k[7:]: v for k, v in hc.items() if k.startswith(tag + "_full.")}
                w, n, a = param_errors(src[tag], ref, names)
                dst[tag + "_worst"], dst[tag + "_worst_name"], dst[tag + "_all"] = w, n, a
                dst.update(dx_figures(tag, src[tag], ref))
            dst["running"] = max(rel(src["buf"][k], gc["buf." + k]) for k in src["buf"] if not k.endswith("num_batches_tracked"))
            assert all(int(src["buf"][k]) == 2 for k in src["buf"] if k.endswith("num_batches_tracked"))
        return fig, floor

    def check_step_is_bit_reproducible(self):
        """Two deterministic discriminator_steps, twice: the same losses, parameters, moments and buffers; NHWC and NCHW inputs are
        the same input; an eval-mode forward moves no statistics and has no backward."""
        gc = self.golden_case(16, 64, 32)
        real, fake = torch.from_numpy(gc["real"]).cuda(), torch.from_numpy(gc["fake"]).cuda()
        runs = []
        for _ in range(2):
            disc = self.network(state=self.init(16), lr=1e-3, deterministic=True)
            outs = [tuple(float(v) for v in disc.discriminator_step(real, nhwc(fake.cpu()), factor=1.0)) for _ in range(2)]
            runs.append((outs, disc.params.cpu().clone(), disc.exp_avg_sq.cpu().clone(), {k: v.cpu().clone() for k, v in disc.buffers.items()}))
            assert disc.global_step == 2 and int(disc.buffers["main.3.num_batches_tracked"]) == 4
            assert float(disc.grads.abs().max()) == 0.0
        assert runs[0][0] == runs[1][0]
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
        assert all(torch.equal(runs[0][3][k], runs[1][3][k]) for k in runs[0][3])
        init = torch.cat([self.init(16)[n].reshape(-1) for n in disc.names])
        assert not torch.equal(runs[0][1], init)
        a, b = self.network(state=self.init(16), deterministic=True), self.network(state=self.init(16), deterministic=True)
        assert torch.equal(a.forward(real), b.forward(nhwc(real.cpu()), layout="nhwc"))
        assert a.logits().shape == (2, 1, 6, 2)
        ev = a.forward(real, training=False)
        assert int(a.buffers["main.3.num_batches_tracked"]) == 1 and torch.isfinite(ev).all()
        with pytest.raises(RuntimeError, match="training-mode forward"):
            a.input_gradient(torch.zeros_like(ev))

    def check_state_round_trip(self, tmp_path):
        """A saved state continues bit for bit in an object built from other weights; the file's keys are STATE_KEYS; a state dict
        with the reference's keys loads, buffers included.  -> (the state dict after two steps, the object built from it).  The
        discriminators own parameters and no tape."""
        from rangeldm_amd.tape import TapeTrainer
        gc = self.golden_case(16, 32, 24)
        real, fake = torch.from_numpy(gc["real"]).cuda(), torch.from_numpy(gc["fake"]).cuda()
        a = self.network(state=self.init(16), lr=1e-3, deterministic=True)
        assert not isinstance(a, TapeTrainer) and not hasattr(a, "_arena")
        a.discriminator_step(real, fake)
        path = str(tmp_path / "d.pt")
        a.save_state(path)
        assert set(torch.load(path, map_location="cpu", weights_only=True)) == self.STATE_KEYS
        a.discriminator_step(real, fake)
        b = self.network(self.config(2, 16, 3), seed=99, lr=1e-3, deterministic=True)
        b.load_state(path)
        assert b.global_step == 1
        b.discriminator_step(real, fake)
        assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(self.module.param_shapes(a.cfg)) and all(torch.equal(sa[k], sb[k]) for k in sa)
        c = self.network(state=sa)
        assert torch.equal(c.buffers["main.9.running_var"].cpu(), sa["main.9.running_var"]) and int(c.buffers["main.6.num_batches_tracked"]) == 4
        return sa, c


PATCH = Family(D, "discriminator.npz", D.DiscriminatorConfig, D.PatchDiscriminator)
META = Family(MK, "metakernel.npz", MK.MetaKernelConfig, MK.MetaKernelDiscriminator)
