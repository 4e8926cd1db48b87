"""CPU: the host half of rangeldm_amd/discriminator.py against the reference's PatchGAN as recorded in
tests/golden/discriminator.npz (tools/make_discriminator_golden.py), and its numpy / torch statements against torch.

Gate of test_forward_host_reproduces_the_golden: forward_host runs the same torch ops as the reference module, so the two differ by
fp32 rounding of differently ordered sums alone.  The golden records the reference against itself with 1 thread and with all
threads (`threads_rel`, 4e-7 .. 1.3e-6 relative L2 where it was written); the gate is max(that, 1e-5) relative L2 per array -- the
1e-5 is the larger of the two everywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rangeldm_amd import discriminator as D
from rangeldm_amd.params import sgm_to_diffusers_vae_key
from tests.disc_util import PATCH as U


def test_keys_are_the_reference_modules():
    keys = [str(k) for k in U.golden()["keys"]]
    assert list(D.param_shapes(D.DiscriminatorConfig())) == keys
    sd = D.init_state(D.DiscriminatorConfig(), 0)
    assert list(sd) == keys
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in D.param_shapes().items())
    assert D.config_from_state(sd) == D.DiscriminatorConfig(2, 64, 3)
    assert [k for k in keys if not k.endswith(D.BUFFER_SUFFIXES)] == D.trainable_names()
    assert sd["main.3.num_batches_tracked"].dtype == torch.int64
    assert D.output_size(None, 1024, 64) == (126, 6) and D.output_size(None, 32, 24) == (2, 1)


def test_init_state_follows_weights_init():
    a, b = D.init_state(None, 3), D.init_state(None, 3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["main.2.weight"], D.init_state(None, 4)["main.2.weight"])
    w = a["main.8.weight"]                                       # 2 M values: the sample moments are tight
    assert abs(float(w.mean())) < 1e-4 and abs(float(w.std()) - 0.02) < 1e-4
    g = a["main.9.weight"]
    assert abs(float(g.mean()) - 1.0) < 5e-3 and abs(float(g.std()) - 0.02) < 3e-3
    assert float(a["main.9.bias"].abs().max()) == 0.0
    bound = 1.0 / np.sqrt(2 * 16)
    assert float(a["main.0.bias"].abs().max()) <= bound and float(a["main.0.bias"].abs().max()) > 0.5 * bound
    assert float(a["main.11.bias"].abs().max()) <= 1.0 / np.sqrt(512 * 16)
    assert float(a["main.3.running_var"].min()) == 1.0 and float(a["main.3.running_mean"].abs().max()) == 0.0


@pytest.mark.parametrize("ndf,W,H", U.CASES)
def test_forward_host_reproduces_the_golden(ndf, W, H):
    gc, hc = U.golden_case(ndf, W, H), U.host_case(ndf, W, H)
    gate = max(float(gc["threads_rel"]), 1e-5)
    worst = {}
    for k in ("logits_real", "logits_fake"):
        assert tuple(hc[k].shape) == gc[k].shape
        worst[k] = U.rel(hc[k], gc[k])
    for k in ("d_loss", "g_loss"):
        worst[k] = abs(hc[k] - float(gc[k])) / abs(float(gc[k]))
    for k, v in gc.items():
        if k.startswith(("d_grad.", "g_grad.")):
            full = hc[k.replace("_grad.", "_full.")]
            worst[k] = U.rel(U.sampled(full), v)
            nk = k.replace("_grad.", "_norm.")
            worst[nk] = abs(float(full.double().norm()) - float(gc[nk])) / (float(gc[nk]) + 1e-30)
        elif k.startswith("buf."):
            if k.endswith("num_batches_tracked"):
                assert int(hc[k]) == int(v) == 2
            else:
                worst[k] = U.rel(hc[k], v)
    assert sum(k.startswith("d_grad.") for k in gc) == len(D.trainable_names()) + 2        # every parameter, both inputs
    assert sum(k.startswith("g_grad.") for k in gc) == len(D.trainable_names()) + 1        # (g does not depend on the real input)
    bad = {k: v for k, v in worst.items() if not v <= gate}
    print(f"ndf {ndf} {W}x{H}: worst {max(worst.values()):.2e} ({max(worst, key=worst.get)}), gate {gate:.1e}")
    assert not bad, bad


def test_bf16_emulation_rounds_only_the_conv_operands():
    """On operands that are exact in bf16 (small integers times a power of two) the emulated conv and its three gradients ARE the
    fp32 conv's; on generic operands they are the conv of the rounded operands, and the bias gradient sums dy unrounded."""
    from tests.hip_util import bf16r, int_grid
    for exact in (True, False):
        if exact:
            x, w, dy = int_grid((2, 16, 6, 5), 1), int_grid((32, 16, 4, 4), 2, -4, 4, exp=-5), int_grid((2, 32, 3, 2), 3)
        else:
            g = torch.Generator().manual_seed(9)
            x, w, dy = (torch.randn(s, generator=g) for s in ((2, 16, 6, 5), (32, 16, 4, 4), (2, 32, 3, 2)))
        b = torch.linspace(-1, 1, 32)
        got, want = [], []
        for emulate, dst in ((True, got), (False, want)):
            xs, ws, bs = ((t if emulate else (bf16r(t) if i < 2 else t)).clone().requires_grad_() for i, t in enumerate((x, w, b)))
            y = D._Bf16Conv.apply(xs, ws, bs, 2) if emulate else F.conv2d(xs, ws, bs, stride=2, padding=1)
            y.backward(dy if emulate else bf16r(dy))
            dst += [y.detach(), xs.grad, ws.grad, bs.grad]
        assert torch.equal(got[0], want[0])
        if exact:
            assert all(torch.equal(a_, b_) for a_, b_ in zip(got, want))
        else:
            # (the plain conv's weight gradient saw bf16(x) and bf16(dy), its data gradient bf16(w) and bf16(dy): the emulation's operands)
            assert U.rel(got[1], want[1]) < 1e-6 and U.rel(got[2], want[2]) < 1e-6
            assert torch.allclose(got[3], dy.sum((0, 2, 3)), rtol=1e-6, atol=1e-6)
            assert not torch.equal(got[3], want[3])              # (the plain run summed the ROUNDED dy)


@pytest.mark.parametrize("shape", [(2, 2, 2, 16), (3, 5, 7, 32), (1, 1, 2, 16)])
def test_batchnorm_host_is_torchs_batch_norm_in_fp64(shape):
    g = torch.Generator().manual_seed(11)
    B, W, H, Cc = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 2 + 0.3
    gamma = 1 + 0.3 * torch.randn(Cc, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(Cc, generator=g, dtype=torch.float64)
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(Cc, generator=g, dtype=torch.float64), torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5
    for training in (True, False):
        xt, gt, bt = (t.clone().requires_grad_() for t in (x, gamma, beta))
        rm_t, rv_t = rm.clone(), rv.clone()
        y = F.leaky_relu(F.batch_norm(xt.permute(0, 3, 1, 2), rm_t, rv_t, gt, bt, training, 0.1, 1e-5), 0.2).permute(0, 2, 3, 1)
        y.backward(dy)
        out = D.batchnorm_host(x.numpy(), gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy(), training, dy.numpy() if training else None)
        assert np.abs(out["y"] - y.detach().numpy()).max() < 1e-12
        if training:
            assert np.abs(out["running_mean"] - rm_t.numpy()).max() < 1e-13 and np.abs(out["running_var"] - rv_t.numpy()).max() < 1e-13
            assert np.abs(out["dx"] - xt.grad.numpy()).max() < 1e-11
            assert np.abs(out["dgamma"] - gt.grad.numpy()).max() < 1e-11 and np.abs(out["dbeta"] - bt.grad.numpy()).max() < 1e-11
    with pytest.raises(ValueError, match="more than 1 value"):
        D.batchnorm_host(np.zeros((1, 1, 1, 4)), np.ones(4), np.zeros(4))


def test_leaky_relu_tie_is_the_slope_side_in_torch():
    """What the kernels and batchnorm_host do at z == 0 -- the gradient 0.2 -- is torch's choice."""
    z = torch.zeros(3, requires_grad=True)
    F.leaky_relu(z, 0.2).sum().backward()
    assert torch.equal(z.grad, torch.full((3,), 0.2))
    out = D.batchnorm_host(np.array([[1.0], [-1.0], [0.0], [0.0]]), np.ones(1), np.zeros(1), dy=np.ones((4, 1)))     # mean 0: z == 0 twice
    assert out["y"][2, 0] == 0.0 and abs(out["dbeta"][0] - (1 + 0.2 * 3)) < 1e-15


def test_hinge_and_adaptive_weight_hosts():
    g = torch.Generator().manual_seed(5)
    real, fake = torch.randn(2, 1, 6, 2, generator=g) * 2, torch.randn(2, 1, 6, 2, generator=g) * 2
    real.view(-1)[:2], fake.view(-1)[:2] = torch.tensor([1.0, -1.0]), torch.tensor([-1.0, 1.0])       # the hinges' corners
    rt, ft = real.clone().requires_grad_(), fake.clone().requires_grad_()
    loss = D.hinge_d_loss_host(rt, ft, factor=0.75)
    loss.backward()
    out, dreal, dfake = D.hinge_host(real.numpy(), fake.numpy(), 0.75)
    assert abs(out[0] - float(loss.detach())) < 1e-6 and abs(out[1] - float(real.mean())) < 1e-6 and abs(out[2] - float(fake.mean())) < 1e-6
    assert np.allclose(dreal, rt.grad.numpy().reshape(-1), rtol=1e-6, atol=0) and np.allclose(dfake, ft.grad.numpy().reshape(-1), rtol=1e-6, atol=0)
    assert dreal[0] == 0.0 and dfake[0] == 0.0                   # relu's gradient at 0 is 0, in torch and here
    a, b = torch.randn(8, generator=g), torch.randn(8, generator=g)
    assert abs(float(D.adaptive_weight_host(a, b, 0.5)) - 0.5 * float(a.norm() / (b.norm() + 1e-4))) < 1e-7
    assert float(D.adaptive_weight_host(a, b * 0, 0.5)) == 0.5 * 1e4                                    # the clamp


def test_sgm_picker_finds_them_and_the_vae_converter_drops_them():
    from rangeldm_amd.checkpoint import convert_sgm_vae_state_dict
    sd = D.init_state(D.DiscriminatorConfig(2, 16, 3), 1)
    for prefix in ("loss.discriminator.", "first_stage_model.loss.discriminator."):
        sgm = {prefix + k: v for k, v in sd.items()}
        sgm[prefix.replace("discriminator.", "logvar")] = torch.zeros(())
        sgm[prefix.replace("loss.discriminator.", "encoder.conv_in.bias")] = torch.zeros(4)
        picked = D.pick_discriminator_state(sgm)
        assert list(picked) == list(sd) and all(picked[k] is sd[k] for k in sd)
        assert D.config_from_state(picked) == D.DiscriminatorConfig(2, 16, 3)
        assert all(sgm_to_diffusers_vae_key(k[len(prefix) - len("loss.discriminator."):]) is None for k in sgm if "discriminator" in k)
        converted = convert_sgm_vae_state_dict(sgm)
        assert list(converted) == ["encoder.conv_in.bias"]
    with pytest.raises(KeyError):
        D.pick_discriminator_state({"encoder.conv_in.bias": torch.zeros(4)})
