"""What the decoder-guidance tests share: the two VAE shapes, the UNet at their latent size, the masks, the operands."""
import numpy as np
import torch

from rangeldm_amd.config import UNetConfig, VAEConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.synth import normal, synth_state_dict

S = VAEConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, sample_size=(64, 16))          # f = 2
TT = VAEConfig(ch=32, ch_mult=(1, 2, 4), num_res_blocks=1, sample_size=(128, 32))     # f = 4
CONFIGS = {"S": S, "T": TT}
LATENT = (4, 32, 8)                                                                    # both: (z_channels, W / f, H / f)
UNET = UNetConfig(sample_size=(32, 8), in_channels=5, out_channels=4, block_out_channels=(32, 32, 64, 64))
MASKS = ("beam4", "beam2", "span", "all", "none")
WC = (40.0, 10.0)


def vae_weights(name):
    return synth_state_dict(vae_param_shapes(CONFIGS[name]), prefix=f"dg/{name}.")


def unet_weights():
    return synth_state_dict(unet_param_shapes(UNET), prefix="dg/unet.")


def mask(kind, W, H):
    """(1, W, H) fp32, 1 = known."""
    m = torch.zeros((1, W, H))
    if kind == "beam4":
        m[..., 2::4] = 1
    elif kind == "beam2":
        m[..., 1::2] = 1
    elif kind == "span":
        m[:, W // 4:] = 1
    elif kind == "all":
        m[:] = 1
    elif kind != "none":
        raise KeyError(kind)
    return m


def mask_pair(first, second, W, H):
    """(2, 1, W, H): a different mask per image."""
    return torch.stack([mask(first, W, H), mask(second, W, H)])


def known_image(seed, B, W, H):
    """(B, 2, W, H): a normalised range profile and a remission, as the drivers' synthetic batch."""
    return torch.from_numpy(normal(seed, "dg/known", (B, 2, W, H))) * 0.5


def latent(seed, B, tag="z"):
    return torch.from_numpy(normal(seed, f"dg/{tag}", (B, *LATENT)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)
