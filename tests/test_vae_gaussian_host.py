"""CPU: the numpy statement of the VAE's posterior (rangeldm_amd.train_ops.gaussian_host, which the device kernels rldm_train_gaussian /
rldm_train_gaussian_backward are tested against) checked with torch autograd of oracle.vae.DiagonalGaussian in fp64; the whole VAE's
parameter plan (rangeldm_amd.vae_training) and the command line's new switches."""
import os

import numpy as np
import pytest
import torch

from oracle.vae import DiagonalGaussian
from rangeldm_amd import train_ops as T
from rangeldm_amd.config import VAEConfig
from rangeldm_amd.params import vae_param_shapes

EDGES = (-31.0, -30.0, 20.0, 21.0)


def _case(B, Z, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(B, 2 * Z, W, H, generator=g, dtype=torch.float64) * 3
    m[0, Z, 0, :4] = torch.tensor(EDGES, dtype=torch.float64)               # logvar below, at and above the clamp's two ends
    noise = torch.randn(B, Z, W, H, generator=g, dtype=torch.float64)
    dz = torch.randn(B, Z, W, H, generator=g, dtype=torch.float64)
    return m, noise, dz


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("sample", [True, False], ids=["sample", "mode"])
@pytest.mark.parametrize("shape", [(3, 4, 5, 4), (1, 1, 1, 4), (2, 3, 7, 6)])
def test_gaussian_host_matches_autograd(shape, sample):
    B, Z, W, H = shape
    m, noise, dz = _case(B, Z, W, H, 11)
    m.requires_grad_()
    kl_weight = 0.37
    d = DiagonalGaussian(m)
    z = d.sample(noise=noise) if sample else d.mode()
    kl = 0.5 * (d.mean ** 2 + torch.exp(d.logvar) - 1 - d.logvar).sum() / B
    (gm,) = torch.autograd.grad((z * dz).sum() + kl_weight * kl, m)
    zh, klh, dmh = T.gaussian_host(_nhwc(m), noise.numpy() if sample else None, _nhwc(dz), kl_weight / B)
    assert zh.dtype == np.float64 and dmh.shape == (B, W, H, 2 * Z)
    assert np.allclose(zh, _nhwc(z), rtol=1e-14, atol=0)
    assert abs(klh - float(kl.detach())) <= 1e-13 * float(kl.detach())
    assert np.allclose(dmh, _nhwc(gm), rtol=1e-12, atol=1e-300)
    # torch's clamp passes the gradient at both ends and nowhere outside
    dl = dmh[0, 0, :4, Z]
    assert dl[0] == 0 and dl[3] == 0 and dl[1] != 0 and dl[2] != 0
    # without dz: no gradient is built
    assert T.gaussian_host(_nhwc(m), None)[2] is None


def test_gaussian_host_in_fp32_is_the_kernel_arithmetic():
    """dtype=np.float32 evaluates every product and sum in fp32: close to the fp64 statement, not equal to it."""
    m, noise, dz = _case(2, 3, 4, 4, 12)
    a = T.gaussian_host(_nhwc(m), noise.numpy(), _nhwc(dz), 0.25, dtype=np.float32)
    b = T.gaussian_host(_nhwc(m), noise.numpy(), _nhwc(dz), 0.25)
    assert a[0].dtype == np.float32 and a[2].dtype == np.float32
    assert np.allclose(a[0], b[0], rtol=1e-5, atol=1e-5) and np.allclose(a[2], b[2], rtol=1e-5, atol=1e-5)
    assert abs(a[1] - b[1]) <= 1e-6 * b[1]


def test_whole_vae_parameter_plan():
    """Every key of vae_param_shapes, the encoder in the order oracle.vae.vae_encode visits it, then decoder_param_names."""
    from rangeldm_amd.vae_training import decoder_param_names, encoder_blocks, encoder_param_names
    cfg = VAEConfig(ch=32, ch_mult=(1, 2, 4), num_res_blocks=2, sample_size=(32, 64))
    shapes = vae_param_shapes(cfg)
    enc, dec = encoder_param_names(cfg, shapes), decoder_param_names(cfg, shapes)
    assert sorted(enc + dec) == sorted(shapes) and len(set(enc + dec)) == len(shapes)
    assert all(n.startswith("encoder.") for n in enc)
    kinds = [k for k, _ in encoder_blocks(cfg)]
    assert kinds == ["conv_in", "resnet", "resnet", "downsample", "resnet", "resnet", "downsample", "resnet", "resnet", "resnet", "resnet",
                     "norm_out", "conv_out"]
    assert enc[:2] == ["encoder.conv_in.weight", "encoder.conv_in.bias"] and enc[-1] == "encoder.conv_out.bias"
    first = "encoder.down_blocks.1.resnets.0."
    block = [n[len(first):] for n in enc if n.startswith(first)]
    assert block == [l + s for l in ("norm1", "conv1", "norm2", "conv_shortcut", "conv2") for s in (".weight", ".bias")]


def test_conv_desc_carries_the_padding_in_its_mode():
    from rangeldm_amd import _lib
    x = torch.zeros(2, 8, 4, 16)
    d = T.conv_desc(x, 32, 9, 2, 0, pad=1)
    assert (d.B, d.Win, d.Hin, d.Cin, d.N, d.taps, d.stride) == (2, 8, 4, 16, 32, 9, 2) and d.mode == _lib.RLDM_TRAIN_PAD_END
    assert T.conv_desc(x, 32, 9, 1, 2, pad=1).mode == 2 | _lib.RLDM_TRAIN_PAD_END
    assert T.conv_desc(x, 32, 9, 2, 0).mode == 0 and T.conv_desc(x, 32, 9, 1, 2, pad=0).mode == 2
    with pytest.raises(ValueError):
        T.conv_desc(x, 32, 9, 2, 0, pad=2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rangeldm_hip.h")).read()
    assert f"#define RLDM_TRAIN_PAD_END {_lib.RLDM_TRAIN_PAD_END}\n" in header


def test_command_line_switches():
    from rangeldm_amd import train_vae as CLI
    base = ["--out", "o", "--steps", "1"]
    a = CLI.build_parser().parse_args(base)
    assert a.trainable == "decoder" and a.kl_weight == 1e-6
    CLI.check_args(a)
    b = CLI.build_parser().parse_args(base + ["--trainable", "all", "--kl-weight", "0.5"])
    assert b.trainable == "all" and b.kl_weight == 0.5
    CLI.check_args(b)
    with pytest.raises(ValueError):
        CLI.check_args(CLI.build_parser().parse_args(base + ["--kl-weight", "-1"]))
    with pytest.raises(SystemExit):
        CLI.build_parser().parse_args(base + ["--trainable", "encoder"])
    assert set(CLI.log_record(3, 1.5, [2.0, 4.0], 2)) == {"step", "loss", "mae"}
    rec = CLI.log_record(3, 1.5, [2.0, 4.0], 2, kl=np.float64(7.0))
    assert rec == {"step": 3, "loss": 1.5, "mae": [1.0, 2.0], "kl": 7.0}
