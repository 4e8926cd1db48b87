"""VAE training on MI355X: the reference's reconstruction phase before its discriminator starts (`GeneralLPIPSWithDiscriminator`
with logvar = 0, perceptual_weight = 0, range_weight = 40, intensity_weight = 10: channel-weighted L1, summed over the image and divided
by the batch) and, with a `discriminator` (discriminator.PatchDiscriminator, or metakernel.MetaKernelDiscriminator: the one the
reference's kitti360.yaml selects), its adversarial phase from `disc_start` on.

`VAEDecoderTrainer` trains the decoder against the frozen encoder.  The latent space does not move: every trained UNet and every
captured sampler stays valid.

`VAETrainer` trains encoder and decoder jointly, as vae/sgm/models/autoencoder.py does: loss = L1 + kl_weight * kl with the
reference's `regularization_weights: {kl_loss: 1e-6}`.  TRAINING THE ENCODER MOVES THE LATENT SPACE: a UNet trained on the old
latents no longer applies to the new VAE, and `scaling_factor` (1 / std of the latents) must be estimated again before one is trained.

Both sit on `TapeTrainer` (tape.py) and drive the op-level HIP kernels of rangeldm_amd/csrc/train*.hip through the same host-side tape as
`UNetTrainer`: 3x3 / 1x1 stride-1 convs, nearest x2 + conv, the encoder's end-padded stride-2 conv (train_ops.conv_desc, pad = 1),
GroupNorm + SiLU, residual adds; the posterior is rldm_train_gaussian, the loss rldm_train_l1.

The adversarial phase (both trainers; `_VAETape._adversarial_step`): the autoencoder's loss becomes nll + d_weight disc_factor g_loss
with g_loss = -mean(D(pred)) and d_weight = clamp(|d nll / d w| / (|d g_loss / d w| + 1e-4), 0, 1e4) disc_weight over
w = decoder.conv_out.weight (the KL term is not part of nll there, as in the reference); then the PatchGAN takes one hinge-loss Adam
step of its own.  ONE DEVIATION, on purpose: the reference runs the autoencoder's forward a second time -- updated weights, a fresh
posterior sample -- for the discriminator's step; here the discriminator sees the reconstruction of the generator's step, which saves
a VAE forward.  `PatchDiscriminator.discriminator_step` is public: a caller who wants the other thing runs it on a fresh forward.

The BEV terms (both trainers; `bev=` a range_image.point_cloud_to_range_image of the images' sensor) rest on a differentiable
`to_voxel`: range_image.to_voxel_train keeps the splat's raw accumulators, to_voxel_backward brings a volume gradient back to the image
in two launches without atomics (rangeldm_amd/csrc/lidar.hip).  The target's volume is the inference `to_voxel`'s, once per step.
  bev_rec_weight > 0   adds (bev_rec_weight / B) sum |V(target)[:, :gz] - V(pred)[:, :gz]| (rldm_train_l1 over the density planes) to
                       the loss; its image-space gradient joins the L1's before the adaptive weight is taken, so it counts in
                       |d nll / d w|.  `last_bev_rec`: the unweighted sum, a 0-d float64 device tensor; the returned loss includes the
                       term.  DEVIATION, on purpose: the reference adds the term to `nll_loss` AFTER `weighted_nll_loss` was formed, so
                       there it reaches the adaptive weight and the log but never the optimised loss.  Here it is a real loss term.
  disc_bev=True        the PatchGAN judges V(pred), all 2 gz planes (a MetaKernelDiscriminator is refused: its range guidance needs a
                       range image); its input gradient returns through to_voxel_backward, and its own step sees (V(target), V(pred)).
SECOND DEVIATION: the reference reassigns `inputs` and `reconstructions` to the volumes once bev_rec_weight > 0, so its discriminator
then sees volumes whatever `disc_bev` says; here the two switches are independent -- pass both to reproduce the reference.
  bev_ordered=True     every BEV volume of the step -- V(pred), V(target), and with them what the discriminator's own step sees -- comes
                       from the order-fixed splat (to_voxel_train(ordered=True), rldm_lidar_to_voxel_ordered: the votes sorted by cell,
                       each cell summed in ascending vote id), slower than the atomic one and the same bits on every run.  With it the
                       BEV terms run under deterministic=True; without it they refuse there (NotImplementedError): the default splat
                       sums its votes with fp32 atomics.  Allowed with deterministic=False (an ordered splat inside an otherwise
                       unordered step); never read when no BEV term is on.

Not built: variant 2 of the Meta-Kernel discriminator and its `log=True` range mapping, the vanilla GAN loss, a trainable `logvar` of the loss (it stays at its initial 0, the reference's `learn_logvar: False`), the perceptual
terms (`bev_perceptual` among them), EMA, a captured step graph, gradient exchange between ranks.  No torch autograd, no torch compute
ops on the path; no CPU fallback.

Parity: tests/test_vae_training_gpu.py and tests/test_vae_encoder_training_gpu.py compare every parameter gradient, and the parameters
after optimizer steps, with torch autograd / torch.optim.Adam on the oracle (oracle/vae.py)."""
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


def encoder_blocks(cfg):
    """The encoder's layers in forward (tape) order, as oracle.vae.vae_encode visits them: [(kind, prefix)], kind in conv_in / resnet /
    downsample / norm_out / conv_out."""
    L = len(cfg.ch_mult)
    out = [("conv_in", "encoder.conv_in")]
    for i in range(L):
        out += [("resnet", f"encoder.down_blocks.{i}.resnets.{j}") for j in range(cfg.num_res_blocks)]
        if i != L - 1:
            out.append(("downsample", f"encoder.down_blocks.{i}.downsamplers.0.conv"))
    return out + [("resnet", "encoder.mid_block.resnets.0"), ("resnet", "encoder.mid_block.resnets.1"),
                  ("norm_out", "encoder.conv_norm_out"), ("conv_out", "encoder.conv_out")]


def _param_names(blocks, shapes, side):
    names = []
    for kind, p in blocks:
        layers = [p]
        if kind == "resnet":
            layers = [p + ".norm1", p + ".conv1", p + ".norm2"]
            if (p + ".conv_shortcut.weight") in shapes:
                layers.append(p + ".conv_shortcut")
            layers.append(p + ".conv2")
        for l in layers:
            names += [l + ".weight", l + ".bias"]
    assert sorted(names) == sorted(k for k in shapes if k.startswith(side))
    return names


def decoder_param_names(cfg, shapes=None):
    """The `decoder.*` keys of vae_param_shapes(cfg) in the order the forward tape first reads them (inside a resnet: norm1, conv1,
    norm2, conv_shortcut, conv2), so backward finishes them in exactly the reverse order."""
    return _param_names(decoder_blocks(cfg), shapes if shapes is not None else vae_param_shapes(cfg), "decoder.")


def encoder_param_names(cfg, shapes=None):
    """The `encoder.*` keys in the order the forward tape first reads them (see decoder_param_names)."""
    return _param_names(encoder_blocks(cfg), shapes if shapes is not None else vae_param_shapes(cfg), "encoder.")


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


class _VAETape(TapeTrainer):
    """What the two VAE trainers share: the hyper-parameters, the resnet block, the decoder walk, the optimizer step and the training
    state."""

    def _init_vae(self, config, state_dict, names, no_dx, *, device, lr, betas, eps, weight_decay, max_grad_norm, channel_weights,
                  deterministic, discriminator, disc_start, disc_weight, disc_factor, bev, bev_rec_weight, disc_bev, bev_ordered):
        """names(cfg, shapes): the trained parameters in tape order; no_dx: TapeTrainer's; the rest: the options both public
        constructors share, under their names there (the defaults stand in those signatures alone)."""
        self._init_bev(bev, bev_rec_weight, disc_bev, deterministic, discriminator, bev_ordered)
        self.cfg = config if isinstance(config, VAEConfig) else VAEConfig(**config)
        if len(channel_weights) != self.cfg.out_channels:
            raise ValueError(f"{len(channel_weights)} channel weights for {self.cfg.out_channels} output channels")
        shapes = vae_param_shapes(self.cfg)
        names = names(self.cfg, shapes)
        trained = set(names)
        self._frozen = OrderedDict((k, v) for k, v in state_dict.items() if k in shapes and k not in trained)
        self._init_parameters(OrderedDict((n, shapes[n]) for n in names), names, state_dict, device, no_dx=no_dx,
                              deterministic=deterministic)
        self.hp = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.channel_weights = torch.tensor([float(w) for w in channel_weights], dtype=torch.float32, device=self.device)
        self.last_abs_sums = None
        self.discriminator, self.disc_start = discriminator, int(disc_start)
        self.disc_weight, self.disc_factor = float(disc_weight), float(disc_factor)
        self.last_g_loss = self.last_d_weight = self.last_disc = None
        self._conv_out_in = None
        if self.bev is not None and (self.disc_bev or self.bev_rec_weight > 0) and int(self.bev.H) != int(self.cfg.sample_size[1]):
            raise ValueError(f"bev is a {self.bev.H}-beam sensor, the VAE's images have H = {self.cfg.sample_size[1]}")

    def _init_bev(self, bev, bev_rec_weight, disc_bev, deterministic, discriminator, bev_ordered):
        """The BEV switches and their refusals (module docstring); with the defaults nothing here is ever read again."""
        self.bev, self.bev_rec_weight, self.disc_bev = bev, float(bev_rec_weight), bool(disc_bev)
        self.bev_ordered = bool(bev_ordered)
        self.last_bev_rec = None
        if self.bev_rec_weight < 0:
            raise ValueError("bev_rec_weight must not be negative")
        if not (self.disc_bev or self.bev_rec_weight > 0):
            return
        if bev is None:
            raise ValueError("disc_bev / bev_rec_weight need bev=, a point_cloud_to_range_image of the images' sensor")
        if deterministic and not self.bev_ordered:
            raise NotImplementedError("the BEV terms are not bit-reproducible: to_voxel's splat sums its votes with fp32 atomics "
                                      "(pass bev_ordered=True for the order-fixed splat)")
        gz = int(bev.grid_sizes[0])
        if self.bev_rec_weight > 0 and gz > 16:
            raise ValueError(f"bev_rec_weight: rldm_train_l1 takes at most 16 density planes, the grid has {gz}")
        if self.disc_bev:
            from .discriminator import PatchDiscriminator
            from .metakernel import MetaKernelDiscriminator                 # (a subclass of PatchDiscriminator)
            if not isinstance(discriminator, PatchDiscriminator) or isinstance(discriminator, MetaKernelDiscriminator):
                raise ValueError("disc_bev needs a discriminator.PatchDiscriminator (the Meta-Kernel discriminator's range guidance "
                                 "needs a range image, not a BEV volume)")
            if discriminator.cfg.in_channels != 2 * gz:
                raise ValueError(f"disc_bev: the BEV volume has {2 * gz} planes, the discriminator takes {discriminator.cfg.in_channels}")

    # ---- network ----------------------------------------------------------------------------------------------
    def _resnet(self, x, p):
        h = self._gn(x, p + ".norm1", True)
        h = self._conv(h, p + ".conv1")
        h = self._gn(h, p + ".norm2", True)
        sc = self._conv(x, p + ".conv_shortcut") if (p + ".conv_shortcut.weight") in self.shapes else x
        return self._conv(h, p + ".conv2", res=sc)

    def _decode(self, h, dz):
        """The decoder on the tape: z (B, W / f, H / f, z_channels) NHWC -> the reconstruction (B, W, H, out_channels) NHWC, kept as
        `_out`.  dz: conv_in computes the gradient of z."""
        for kind, p in decoder_blocks(self.cfg):
            if kind == "resnet":
                h = self._resnet(h, p)
            elif kind == "norm_out":
                h = self._gn(h, p, True)
            else:
                if kind == "conv_out":
                    self._conv_out_in = h               # (the adversarial phase takes conv_out's weight gradient twice more)
                h = self._conv(h, p, mode=1 if kind == "upsample" else 0, need_dx=dz or kind != "conv_in")
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

    # ---- adversarial phase ------------------------------------------------------------------------------------
    def adversarial(self):
        """True when the next train_step runs the adversarial phase: a discriminator was given and global_step (the steps taken so
        far) has reached disc_start -- the reference's adopt_weight(disc_factor, global_step, threshold=disc_start)."""
        return self.discriminator is not None and self.global_step >= self.disc_start

    # ---- BEV terms ----------------------------------------------------------------------------------------------
    def _bev_active(self):
        return self.bev_rec_weight > 0 or (self.disc_bev and self.adversarial())

    def _bev_volumes(self, pred, target_nchw):
        """-> (V(target): the inference to_voxel, no gradient; V(pred), saved: to_voxel_train of the reconstruction)."""
        vt = self.bev.to_voxel(target_nchw, ordered=self.bev_ordered)
        vp, saved = self.bev.to_voxel_train(T.unpack_output(pred), ordered=self.bev_ordered)
        return vt, vp, saved

    def _bev_rec(self, dpred, volumes):
        """The term (bev_rec_weight / B) sum |V(target)[:, :gz] - V(pred)[:, :gz]|: rldm_train_l1 over the density planes, its gradient
        brought to image space by to_voxel_backward and added to dpred.  -> (dpred, the weighted term); last_bev_rec = the
        unweighted sum, a 0-d float64 device tensor."""
        vt, vp, saved = volumes
        gz = int(self.bev.grid_sizes[0])
        wc = torch.full((gz,), self.bev_rec_weight, dtype=torch.float32, device=self.device)
        term, dplanes, sums = T.l1(T.pack_input(vp[:, :gz].contiguous(), False), vt[:, :gz].contiguous(), wc)
        self.last_bev_rec = sums.sum()
        dvox = torch.zeros_like(vp)
        dvox[:, :gz] = T.unpack_output(dplanes)
        return T.add(dpred, T.pack_input(self.bev.to_voxel_backward(saved, dvox), False)), term

    def _adversarial_step(self, pred, dnll, real_nchw, volumes=None):
        """The steps behind the forward and the L1 of an adversarial train_step (module docstring): generator term through the
        discriminator (training-mode BatchNorm, as the reference), the adaptive weight from two weight gradients of conv_out alone,
        one backward with the mixed gradient, the VAE's Adam step, then the discriminator's own step on (real, pred) with the
        trainer's step count.  Sets last_g_loss / last_d_weight / last_disc = (d_loss, mean logits real, mean logits fake): device
        scalars, no host sync."""
        from . import discriminator as D
        disc = self.discriminator
        if self.disc_bev:       # the discriminator judges the BEV volume: its input gradient comes back through to_voxel_backward
            vt, vp, saved = volumes
            disc.forward(vp, training=True, layout="nchw")
            self.last_g_loss, dlogits = disc.generator_loss()
            dg = T.pack_input(self.bev.to_voxel_backward(saved, T.unpack_output(disc.input_gradient(dlogits))), False)
            real_nchw, pred = vt, vp
        else:
            disc.forward(pred, training=True, layout="nhwc")
            self.last_g_loss, dlogits = disc.generator_loss()
            dg = disc.input_gradient(dlogits)
        w = "decoder.conv_out.weight"
        sq = []
        for d in (dnll, dg):
            gw = torch.zeros(self.shapes[w], dtype=torch.float32, device=self.device)
            T.wgrad(d, self._conv_out_in, gw, 9)
            sq.append(T.sqnorm(gw))
        dpred, self.last_d_weight = D.adaptive_mix(dnll, dg, sq[0], sq[1], self.disc_weight, self.disc_factor)
        self.backward(dpred)
        self.optimizer_step()
        self.last_disc = disc.discriminator_step(real_nchw, pred, factor=self.disc_factor, step=self.global_step)

    def _reconstruction_step(self, pred, target):
        """What a train_step does behind its forward: the L1 against target (sets last_abs_sums), the BEV volumes and term when they
        are on, then the adversarial phase's step or backward + optimizer step.  -> the reconstruction loss (L1 + the BEV term)."""
        rec, dpred, self.last_abs_sums = T.l1(pred, target, self.channel_weights)
        volumes = None
        if self._bev_active():
            volumes = self._bev_volumes(pred, target)
            if self.bev_rec_weight > 0:
                dpred, term = self._bev_rec(dpred, volumes)
                rec = rec + term
        if self.adversarial():
            self._adversarial_step(pred, dpred, target, volumes)
        else:
            self.backward(dpred)
            self.optimizer_step()
        return rec

    # ---- weights ----------------------------------------------------------------------------------------------
    def full_state_dict(self):
        """The whole VAE: the tensors this trainer does not train as they were given, the fp32 masters of those it does."""
        return merged_state_dict(self._frozen, self.state_dict())

    def state_payload(self):
        """Everything a resumed run needs: parameters, Adam moments, step counter -- and, with a discriminator, its state under the
        key `discriminator` (a file written without one has no such key)."""
        st = super().state_payload()
        if self.discriminator is not None:
            st["discriminator"] = self.discriminator.state_payload()
        return st

    def load_payload(self, st):
        super().load_payload(st)
        if self.discriminator is not None and "discriminator" in st:
            self.discriminator.load_payload(st["discriminator"])


class VAEDecoderTrainer(_VAETape):
    def __init__(self, config, state_dict, device="cuda", lr=4.5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, channel_weights=(40.0, 10.0), deterministic=False, discriminator=None, disc_start=0,
                 disc_weight=0.5, disc_factor=1.0, bev=None, bev_rec_weight=0.0, disc_bev=False, bev_ordered=False):
        """The defaults are the reference's: torch.optim.Adam (AdamW with zero decay is Adam) at base_learning_rate 4.5e-6, no
        clipping, range_weight 40 / intensity_weight 10.  state_dict may hold the whole VAE: the encoder's tensors are kept as
        they are (handed on by load_into / save_pretrained), never read by a kernel of this class.
        deterministic: every kernel of this trainer runs in the library's deterministic mode (rldm_train_deterministic), as
        UNetTrainer(deterministic=True): the same inputs give the same parameter bits.
        discriminator: a discriminator.PatchDiscriminator or a metakernel.MetaKernelDiscriminator; from step disc_start on train_step
        runs the adversarial phase (module docstring) with disc_weight / disc_factor, the reference's names.  None, or before
        disc_start: the step is exactly what it is without one, and the discriminator is not run.
        bev, bev_rec_weight, disc_bev, bev_ordered: the BEV terms (module docstring); with the defaults no code of theirs runs."""
        self._init_vae(config, state_dict, decoder_param_names, ("decoder.conv_in.weight",), device=device, lr=lr, betas=betas, eps=eps,
                       weight_decay=weight_decay, max_grad_norm=max_grad_norm, channel_weights=channel_weights,
                       deterministic=deterministic, discriminator=discriminator, disc_start=disc_start, disc_weight=disc_weight,
                       disc_factor=disc_factor, bev=bev, bev_rec_weight=bev_rec_weight, disc_bev=disc_bev, bev_ordered=bev_ordered)

    def forward(self, z_nchw):
        """z (B, z_channels, W / f, H / f) fp32 on the device, as the encoder emits it (not multiplied by scaling_factor)
        -> the reconstruction (B, W, H, out_channels) NHWC.  Records the tape for `backward`."""
        with self._mode():
            if z_nchw.shape[1] != self.cfg.z_channels:
                raise ValueError(f"latent has {z_nchw.shape[1]} channels, the decoder expects {self.cfg.z_channels}")
            self._begin_tape()
            return self._decode(T.pack_input(z_nchw.to(self.device).float().contiguous(), False), dz=False)

    def train_step(self, z_nchw, target_nchw, as_float=False):
        """pred = decoder(z); loss = (1 / B) sum wc[c] |pred - target|; backward; step.  Returns the loss: a 0-d float64 device
        tensor (no host sync), or a Python float with as_float.  `last_abs_sums`: float64 (C,) device, the unweighted sum of
        |pred - target| per channel (MAE of channel c = last_abs_sums[c] / (B W H)).  In the adversarial phase (`adversarial()`) the
        step is `_adversarial_step`'s and `last_g_loss`, `last_d_weight`, `last_disc` report it; the returned loss stays the L1."""
        with self._mode():
            pred = self.forward(z_nchw)
            loss = self._reconstruction_step(pred, target_nchw.to(self.device).float().contiguous())
        return float(loss) if as_float else loss

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


class VAETrainer(_VAETape):
    def __init__(self, config, state_dict, device="cuda", lr=4.5e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, kl_weight=1e-6, channel_weights=(40.0, 10.0), deterministic=False, discriminator=None,
                 disc_start=0, disc_weight=0.5, disc_factor=1.0, bev=None, bev_rec_weight=0.0, disc_bev=False, bev_ordered=False):
        """Encoder and decoder trained jointly; the defaults are the reference's (VAEDecoderTrainer's, and kl_loss: 1e-6).  The
        parameters are every key of vae_param_shapes in tape order: the encoder as oracle.vae.vae_encode visits it, then the
        decoder.  Training the encoder moves the latent space: UNets trained on the old latents no longer apply, and scaling_factor
        must be estimated again (module docstring).  deterministic, discriminator, disc_start, disc_weight, disc_factor, bev,
        bev_rec_weight, disc_bev, bev_ordered: as VAEDecoderTrainer."""
        self._init_vae(config, state_dict, lambda cfg, shapes: encoder_param_names(cfg, shapes) + decoder_param_names(cfg, shapes),
                       ("encoder.conv_in.weight",), device=device, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                       max_grad_norm=max_grad_norm, channel_weights=channel_weights, deterministic=deterministic,
                       discriminator=discriminator, disc_start=disc_start, disc_weight=disc_weight, disc_factor=disc_factor, bev=bev,
                       bev_rec_weight=bev_rec_weight, disc_bev=disc_bev, bev_ordered=bev_ordered)
        self.kl_weight = float(kl_weight)
        self.last_kl = None
        self._moments = self._z = None

    def _encode(self, h):
        for kind, p in encoder_blocks(self.cfg):
            if kind == "resnet":
                h = self._resnet(h, p)
            elif kind == "norm_out":
                h = self._gn(h, p, True)
            elif kind == "downsample":
                h = self._conv(h, p, stride=2, pad=1)
            else:
                h = self._conv(h, p, need_dx=kind != "conv_in")
        return h

    def _gaussian(self, moments, noise):
        """z = mean + std noise (noise None: z = mean) and the KL term on the tape; backward adds kl_weight d(kl) / d(moments)."""
        z, self.last_kl = T.gaussian(moments, noise)
        kw = self.kl_weight / moments.shape[0]

        def bwd():
            self._acc(moments, T.gaussian_backward(moments, noise, self._pop(z), kw), True)
        self._tape.append(bwd)
        return z

    def forward(self, images, noise=None):
        """images (B, in_channels, W, H) fp32; noise (B, z_channels, W / f, H / f), or None for z = mean -> the reconstruction
        (B, W, H, out_channels) NHWC.  Records the tape for `backward`; `last_kl` and `moments()` are this pass's."""
        with self._mode():
            if images.shape[1] != self.cfg.in_channels:
                raise ValueError(f"images have {images.shape[1]} channels, the encoder expects {self.cfg.in_channels}")
            self._begin_tape()
            self._moments = self._encode(T.pack_input(images.to(self.device).float().contiguous(), False))
            if noise is not None:
                noise = noise.to(self.device).float().contiguous()
            self._z = self._gaussian(self._moments, noise)
            return self._decode(self._z, dz=True)

    def moments(self):
        """The last forward's moments as (B, 2 z_channels, W / f, H / f): [mean | logvar], what `vae.encode` returns."""
        return T.unpack_output(self._moments)

    def latents(self):
        """The last forward's z as (B, z_channels, W / f, H / f): what its decoder saw."""
        return T.unpack_output(self._z)

    def train_step(self, images, noise=None, generator=None, sample_posterior=True, as_float=False, sample_offset=0):
        """moments = encoder(images); z = mean + std noise (sample_posterior=False: z = mean); pred = decoder(z);
        loss = (1 / B) sum wc[c] |pred - images| + kl_weight kl; backward through decoder, posterior and encoder; one Adam step over
        all parameters.  noise: (B, z_channels, W / f, H / f); None draws it on the host from `generator`, as the reference does, or
        on the device when `generator` is a rng.DeviceGenerator (rng.randn, one draw, at `sample_offset`).
        Returns the loss: a 0-d float64 device tensor (no host sync), or a Python float with as_float.  `last_abs_sums` as
        VAEDecoderTrainer's; `last_kl`: the KL term, a 0-d float64 device tensor.  In the adversarial phase: as VAEDecoderTrainer's
        (the returned loss stays L1 + kl_weight kl; the discriminator is given `images` as the real batch)."""
        images = images.to(self.device).float().contiguous()
        if sample_posterior and noise is None:
            from .rng import DeviceGenerator, randn
            f = self.cfg.downscale
            zshape = (images.shape[0], self.cfg.z_channels, images.shape[2] // f, images.shape[3] // f)
            if isinstance(generator, DeviceGenerator):
                noise = randn(zshape, generator, sample_offset, self.device)
            else:
                noise = torch.randn(zshape, generator=generator)
        with self._mode():
            pred = self.forward(images, noise if sample_posterior else None)
            rec = self._reconstruction_step(pred, images)
        loss = rec + self.kl_weight * self.last_kl          # (two device scalars, for the log: no kernel reads the sum)
        return float(loss) if as_float else loss

    def load_into(self, vae):
        """Hand the trained VAE to an AutoencoderKLHIP (see VAEDecoderTrainer.load_into)."""
        return vae.load_state_dict(self.full_state_dict())

    def save_pretrained(self, output_dir):
        """`output_dir/vae/` as AutoencoderKLHIP.from_pretrained reads it."""
        save_vae_dir(output_dir, self.cfg, self.full_state_dict())


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
