"""VAE decoder fine-tuning on MI355X: the decoder of the range-image VAE trained against its frozen encoder with the reference's
reconstruction term before the discriminator starts (channel-weighted L1, summed over the image and divided by the batch --
`GeneralLPIPSWithDiscriminator` with logvar = 0, perceptual_weight = 0, range_weight = 40, intensity_weight = 10).  The latent
space does not move: every trained UNet and every captured sampler stays valid.

`VAEDecoderTrainer` (on `TapeTrainer`, tape.py) drives the op-level HIP kernels of rangeldm_amd/csrc/train.hip through the same
host-side tape as `UNetTrainer`: 3x3 / 1x1 stride-1 convs, nearest x2 + conv, GroupNorm + SiLU, residual adds; the loss is
rldm_train_l1.  Not built: encoder gradients and the KL term (the training convs have no end-only padding, which the encoder's two
down-samplers use), the discriminator, EMA, a captured step graph, gradient exchange between ranks.  No torch autograd, no torch
compute ops on the path; no CPU fallback.

Parity: tests/test_vae_training_gpu.py compares every parameter gradient, and the parameters after optimizer steps, with torch
autograd / torch.optim.Adam on the oracle (oracle/vae.py)."""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import train_ops as T
from .config import VAEConfig
from .params import vae_param_shapes
from .tape import TapeTrainer


def decoder_blocks(cfg):
    """The decoder's layers in forward (tape) order: [(kind, prefix)], kind in conv_in / resnet / upsample / norm_out / conv_out."""
    L = len(cfg.ch_mult)
    out = [("conv_in", "decoder.conv_in"), ("resnet", "decoder.mid_block.resnets.0"), ("resnet", "decoder.mid_block.resnets.1")]
    for i in range(L):
        out += [("resnet", f"decoder.up_blocks.{i}.resnets.{j}") for j in range(cfg.num_res_blocks + 1)]
        if i != L - 1:
            out.append(("upsample", f"decoder.up_blocks.{i}.upsamplers.0.conv"))
    return out + [("norm_out", "decoder.conv_norm_out"), ("conv_out", "decoder.conv_out")]


def decoder_param_names(cfg, shapes=None):
    """The `decoder.*` keys of vae_param_shapes(cfg) in the order the forward tape first reads them (inside a resnet: norm1, conv1,
    norm2, conv_shortcut, conv2), so backward finishes them in exactly the reverse order."""
    shapes = shapes if shapes is not None else vae_param_shapes(cfg)
    names = []
    for kind, p in decoder_blocks(cfg):
        layers = [p]
        if kind == "resnet":
            layers = [p + ".norm1", p + ".conv1", p + ".norm2"]
            if (p + ".conv_shortcut.weight") in shapes:
                layers.append(p + ".conv_shortcut")
            layers.append(p + ".conv2")
        for l in layers:
            names += [l + ".weight", l + ".bias"]
    assert sorted(names) == sorted(k for k in shapes if k.startswith("decoder."))
    return names


def merged_state_dict(encoder_source, decoder_sd):
    """The whole VAE's state dict: every non-decoder tensor of `encoder_source` as it is, the decoder's from `decoder_sd`."""
    out = OrderedDict((k, v) for k, v in encoder_source.items() if not k.startswith("decoder."))
    out.update(decoder_sd)
    return out


def save_vae_dir(output_dir, cfg, state_dict):
    """`output_dir/vae/` in the layout AutoencoderKLHIP.from_pretrained (and `evaluate vae --weights output_dir`) reads."""
    from .checkpoint import save_model_dir, vae_config_to_diffusers
    sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
    save_model_dir(os.path.join(output_dir, "vae"), vae_config_to_diffusers(cfg), sd)


class VAEDecoderTrainer(TapeTrainer):
    def __init__(self, config, state_dict, device="cuda", lr=4.5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, channel_weights=(40.0, 10.0), deterministic=False):
        """The defaults are the reference's: torch.optim.Adam (AdamW with zero decay is Adam) at base_learning_rate 4.5e-6, no
        clipping, range_weight 40 / intensity_weight 10.  state_dict may hold the whole VAE: the encoder's tensors are kept as
        they are (handed on by load_into / save_pretrained), never read by a kernel of this class.
        deterministic: every kernel of this trainer runs in the library's deterministic mode (rldm_train_deterministic), as
        UNetTrainer(deterministic=True): the same inputs give the same parameter bits."""
        self.cfg = config if isinstance(config, VAEConfig) else VAEConfig(**config)
        if len(channel_weights) != self.cfg.out_channels:
            raise ValueError(f"{len(channel_weights)} channel weights for {self.cfg.out_channels} output channels")
        shapes = vae_param_shapes(self.cfg)
        names = decoder_param_names(self.cfg, shapes)
        self._frozen = OrderedDict((k, v) for k, v in state_dict.items() if k in shapes and not k.startswith("decoder."))
        self._init_parameters(OrderedDict((n, shapes[n]) for n in names), names, state_dict, device,
                              no_dx=("decoder.conv_in.weight",), deterministic=deterministic)
        self.hp = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.channel_weights = torch.tensor([float(w) for w in channel_weights], dtype=torch.float32, device=self.device)
        self.last_abs_sums = None

    # ---- network ----------------------------------------------------------------------------------------------
    def _resnet(self, x, p):
        h = self._gn(x, p + ".norm1", True)
        h = self._conv(h, p + ".conv1")
        h = self._gn(h, p + ".norm2", True)
        sc = self._conv(x, p + ".conv_shortcut") if (p + ".conv_shortcut.weight") in self.shapes else x
        return self._conv(h, p + ".conv2", res=sc)

    def forward(self, z_nchw):
        """z (B, z_channels, W / f, H / f) fp32 on the device, as the encoder emits it (not multiplied by scaling_factor)
        -> the reconstruction (B, W, H, out_channels) NHWC.  Records the tape for `backward`."""
        with self._mode():
            if z_nchw.shape[1] != self.cfg.z_channels:
                raise ValueError(f"latent has {z_nchw.shape[1]} channels, the decoder expects {self.cfg.z_channels}")
            self._begin_tape()
            h = T.pack_input(z_nchw.to(self.device).float().contiguous(), False)
            for kind, p in decoder_blocks(self.cfg):
                if kind == "resnet":
                    h = self._resnet(h, p)
                elif kind == "norm_out":
                    h = self._gn(h, p, True)
                else:
                    h = self._conv(h, p, mode=1 if kind == "upsample" else 0, need_dx=kind != "conv_in")
            self._out = h
            return h

    def sample_nchw(self):
        """The last forward's reconstruction as (B, out_channels, W, H)."""
        return T.unpack_output(self._out)

    def backward(self, dpred_nhwc):
        """Replays the tape in reverse: the flat gradient buffer += d(loss) / d(parameters) for d(loss) / d(pred) = dpred."""
        with self._mode():
            self._run_tape(self._out, dpred_nhwc)

    def optimizer_step(self):
        """(clip_grad_norm_ when max_grad_norm is set) + Adam at the constant rate, then the bf16 operand copies are refreshed and
        the gradients zeroed."""
        with self._mode():
            self.global_step += 1
            self._clip_adamw(self.hp["lr"])
            return self.hp["lr"]

    def train_step(self, z_nchw, target_nchw, as_float=False):
        """pred = decoder(z); loss = (1 / B) sum wc[c] |pred - target|; backward; step.  Returns the loss: a 0-d float64 device
        tensor (no host sync), or a Python float with as_float.  `last_abs_sums`: float64 (C,) device, the unweighted sum of
        |pred - target| per channel (MAE of channel c = last_abs_sums[c] / (B W H))."""
        with self._mode():
            pred = self.forward(z_nchw)
            loss, dpred, self.last_abs_sums = T.l1(pred, target_nchw.to(self.device).float().contiguous(), self.channel_weights)
            self.backward(dpred)
            self.optimizer_step()
        return float(loss) if as_float else loss

    # ---- weights ----------------------------------------------------------------------------------------------
    def full_state_dict(self):
        """The whole VAE: the frozen encoder's tensors as they were given, the decoder's fp32 masters."""
        return merged_state_dict(self._frozen, self.state_dict())

    def load_into(self, vae):
        """Hand the trained decoder (and the unchanged encoder) to an AutoencoderKLHIP: its load_state_dict advances the VAE's
        generation counter, so every sampler built on it plans again."""
        enc = self._frozen if self._frozen else {k: v for k, v in vae.state_dict().items() if not k.startswith("decoder.")}
        return vae.load_state_dict(merged_state_dict(enc, self.state_dict()))

    def save_pretrained(self, output_dir):
        """`output_dir/vae/` as AutoencoderKLHIP.from_pretrained reads it; the encoder's weights pass through from the state dict
        the trainer was given."""
        if not self._frozen:
            raise RuntimeError("save_pretrained writes a whole VAE: the trainer was built from decoder weights only")
        save_vae_dir(output_dir, self.cfg, self.full_state_dict())

    def save_state(self, path):
        """Everything a resumed run needs: parameters, Adam moments, step counter."""
        torch.save({"params": self.params.cpu(), "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
                    "global_step": self.global_step, "names": list(self.names)}, path)

    def load_state(self, path):
        st = torch.load(path, map_location="cpu", weights_only=True)
        if list(st["names"]) != list(self.names):
            raise RuntimeError("training state was saved for a different parameter layout")
        self.params.copy_(st["params"])
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.global_step = int(st["global_step"])
        self.grads.zero_()
        self.repack()


def training_step(trainer, vae, images, sample_posterior=True, generator=None, noise=None, as_float=False):
    """One iteration of the reconstruction phase with a frozen encoder: z = vae.encode(images).latent_dist.sample() (or .mode()),
    NOT multiplied by scaling_factor -- the decoder sees what the encoder emits, as in AutoencodingEngine.forward -- on the
    inference kernels, no gradient; then trainer.train_step(z, images).  In the trainer's deterministic mode the decoder's forward /
    loss / backward / optimizer are bit-reproducible (the encode and the noise draw are outside that guarantee; pass `noise`)."""
    images = images.to(trainer.device).float()
    with torch.no_grad():
        dist = vae.encode(images).latent_dist
        z = dist.sample(generator=generator, noise=noise) if sample_posterior else dist.mode().contiguous()
    return trainer.train_step(z, images, as_float=as_float)
