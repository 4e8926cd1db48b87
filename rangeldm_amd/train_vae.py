"""python -m rangeldm_amd.train_vae: fine-tune the VAE's decoder against its frozen encoder, or the whole VAE (rangeldm_amd/vae_training.py).

    python -m rangeldm_amd.train_vae --weights DIR | --sgm-ckpt F --sgm-yaml Y  [--input NPY_DIR] --out DIR --steps N
                                     [--trainable decoder|all] [--kl-weight 1e-6]
                                     [--batch-size 8] [--lr 4.5e-6] [--mode] [--seed S] [--log-every K] [--deterministic]
                                     [--discriminator patchgan|metakernel --disc-start N --disc-weight 0.5 [--disc-state FILE]]
                                     [--disc-bev] [--bev-rec-weight X] [--bev-ordered] [--bev-grid D H W] [--bev-range x0 y0 z0 x1 y1 z1]

--trainable decoder (the default) leaves the encoder, and with it the latent space, as it is.  --trainable all trains encoder and
decoder jointly with loss = L1 + kl_weight * kl and adds "kl" to every log line; it moves the latent space, so UNets trained on the old
latents no longer apply and scaling_factor must be estimated again.

--discriminator patchgan adds the reference's adversarial phase (rangeldm_amd/discriminator.py) from step --disc-start on: every log
line of that phase gains "g_loss", "d_weight", "disc_loss", "logits_real", "logits_fake", and OUT/discriminator.pt (PatchDiscriminator's
save_state; --disc-state FILE resumes from one) is written beside OUT/vae/.  --discriminator metakernel does the same against the
range-guided Meta-Kernel discriminator that the reference's kitti360.yaml selects (rangeldm_amd/metakernel.py,
MetaKernelDiscriminator).  Without the option the command prints and writes what it always did.

--bev-rec-weight X adds the BEV density term of rangeldm_amd/vae_training.py to the loss and "bev_rec" (the unweighted sum of
|V(target) - V(pred)| over the density planes) to every log line; --disc-bev (with --discriminator patchgan) hands the PatchGAN the BEV
volume of the reconstruction instead of the range image.  The volume is --bev-grid / --bev-range (defaults: the reference's
kitti360.yaml); the sensor follows the image height: 64 beams KITTI-360, 32 nuScenes.  --bev-ordered forms every BEV volume with the
order-fixed splat (bev_ordered=True: slower, the same bits on every run); --deterministic takes the BEV flags only together with it.

--input holds the (2, W, H) .npy range images `evaluate vae --input` reads (batches walk the sorted files and wrap around); without
it the run trains on the synthetic batch of `evaluate vae`.  Without --weights / --sgm-ckpt the synthetic weights of `evaluate vae`
are trained (a plumbing check).  One JSON line per --log-every steps: {"step", "loss", "mae": [per channel]}; the result is written
to OUT/vae/, which `evaluate vae --weights OUT` reads."""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m rangeldm_amd.train_vae", description=__doc__.split("\n")[0])
    ap.add_argument("--weights", default=None, help="diffusers VAE directory, or a training output_dir holding vae/")
    ap.add_argument("--sgm-ckpt", default=None, help="sgm AutoencodingEngine .ckpt")
    ap.add_argument("--sgm-yaml", default=None, help="the yaml the sgm checkpoint was trained with")
    ap.add_argument("--input", default=None, help="directory of (2, W, H) .npy range images (default: synthetic batch)")
    ap.add_argument("--out", required=True, help="output directory: OUT/vae/ is written")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--trainable", choices=("decoder", "all"), default="decoder",
                    help="decoder: the encoder stays frozen; all: encoder + decoder with the KL term (moves the latent space)")
    ap.add_argument("--kl-weight", type=float, default=1e-6, help="weight of the KL term (--trainable all)")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--lr", type=float, default=4.5e-6)
    ap.add_argument("--mode", action="store_true", help="decode the posterior's mode instead of a sample")
    ap.add_argument("--seed", type=int, default=20240310)
    ap.add_argument("--log-every", type=int, default=10, metavar="K")
    ap.add_argument("--deterministic", action="store_true", help="bit-reproducible decoder step (slower)")
    ap.add_argument("--discriminator", choices=("patchgan", "metakernel"), default=None,
                    help="train adversarially from --disc-start on against the PatchGAN or the Meta-Kernel discriminator")
    ap.add_argument("--disc-start", type=int, default=0, metavar="N", help="first step (0-based) of the adversarial phase")
    ap.add_argument("--disc-weight", type=float, default=0.5, help="factor of the adaptive weight")
    ap.add_argument("--disc-state", default=None, metavar="FILE", help="a discriminator.pt to resume the discriminator from")
    ap.add_argument("--disc-bev", action="store_true", help="the PatchGAN judges the BEV volume of the reconstruction")
    ap.add_argument("--bev-rec-weight", type=float, default=0.0, metavar="X", help="weight of the BEV density L1 term (0: off)")
    ap.add_argument("--bev-ordered", action="store_true", help="order-fixed BEV splat: bit-reproducible BEV terms (slower)")
    ap.add_argument("--bev-grid", type=int, nargs=3, default=[1, 512, 512], metavar=("D", "H", "W"), help="grid_sizes of the BEV volume")
    ap.add_argument("--bev-range", type=float, nargs=6, default=[-51.2, -51.2, -3.0, 51.2, 51.2, 1.0],
                    metavar=("x0", "y0", "z0", "x1", "y1", "z1"), help="pc_range of the BEV volume [m]")
    return ap


def check_args(a):
    if a.steps < 1 or a.batch_size < 1 or a.log_every < 1:
        raise ValueError("--steps, --batch-size and --log-every must be at least 1")
    if a.kl_weight < 0:
        raise ValueError("--kl-weight must not be negative")
    if a.weights and a.sgm_ckpt:
        raise ValueError("--weights and --sgm-ckpt exclude each other")
    if a.sgm_yaml and not a.sgm_ckpt:
        raise ValueError("--sgm-yaml goes with --sgm-ckpt")
    if a.disc_start < 0 or a.disc_weight < 0:
        raise ValueError("--disc-start and --disc-weight must not be negative")
    if a.disc_state and not a.discriminator:
        raise ValueError("--disc-state goes with --discriminator")
    if a.bev_rec_weight < 0:
        raise ValueError("--bev-rec-weight must not be negative")
    if a.disc_bev and a.discriminator != "patchgan":
        raise ValueError("--disc-bev goes with --discriminator patchgan (the Meta-Kernel discriminator needs a range image)")
    if (a.disc_bev or a.bev_rec_weight > 0) and a.deterministic and not a.bev_ordered:
        raise ValueError("--disc-bev / --bev-rec-weight do not run with --deterministic (the BEV splat sums with fp32 atomics) "
                         "unless --bev-ordered is given")
    if min(a.bev_grid) < 1 or any(a.bev_range[i + 3] <= a.bev_range[i] for i in range(3)):
        raise ValueError("--bev-grid must be positive and --bev-range must be x0 y0 z0 x1 y1 z1 with x0 < x1, y0 < y1, z0 < z1")


def log_record(step, loss, abs_sums, pixels, kl=None, adversarial=None, bev=None):
    """One log line: the loss of `step` (1-based) and the per-channel MAE = abs_sums[c] / pixels (pixels = B W H); kl (--trainable all):
    the KL term, unweighted; adversarial (once that phase has started): (g_loss, d_weight, (disc_loss, logits_real, logits_fake)); bev
    (--bev-rec-weight): the trainer's last_bev_rec, logged as "bev_rec"."""
    rec = {"step": int(step), "loss": float(loss), "mae": [float(s) / float(pixels) for s in abs_sums]}
    if kl is not None:
        rec["kl"] = float(kl)
    if adversarial is not None:
        g_loss, d_weight, (disc_loss, logits_real, logits_fake) = adversarial
        rec.update(g_loss=float(g_loss), d_weight=float(d_weight), disc_loss=float(disc_loss), logits_real=float(logits_real),
                   logits_fake=float(logits_fake))
    if bev is not None:
        rec["bev_rec"] = float(bev)
    return rec


def bev_sensor(height, width, grid, pc_range):
    """The point_cloud_to_range_image of the sensor with `height` beams (64: KITTI-360, 32: nuScenes) over the given BEV volume."""
    from .range_image import point_cloud_to_range_image_KITTI, point_cloud_to_range_image_nuScenes
    sensors = {64: point_cloud_to_range_image_KITTI, 32: point_cloud_to_range_image_nuScenes}
    if height not in sensors:
        raise ValueError(f"no sensor with {height} beams: the BEV terms need images of height 64 (KITTI-360) or 32 (nuScenes)")
    return sensors[height](width=int(width), grid_sizes=[int(g) for g in grid], pc_range=[float(v) for v in pc_range])


def batch_files(files, step, batch_size):
    """The files of batch `step` (0-based): consecutive, wrapping around the sorted list."""
    n = len(files)
    return [files[(step * batch_size + i) % n] for i in range(batch_size)]


def load_model(a):
    """(VAEConfig, whole state dict) from --weights / --sgm-ckpt, or the synthetic weights."""
    from .checkpoint import load_sgm_vae_checkpoint, load_vae_dir
    if a.sgm_ckpt:
        return load_sgm_vae_checkpoint(a.sgm_ckpt, a.sgm_yaml)
    if a.weights:
        sub = os.path.join(a.weights, "vae")
        return load_vae_dir(sub if os.path.isdir(sub) else a.weights)
    from .config import VAEConfig
    from .params import vae_param_shapes
    from .synth import synth_state_dict
    cfg = VAEConfig()
    return cfg, synth_state_dict(vae_param_shapes(cfg), seed=a.seed, prefix="vae.")


def main(argv=None):
    a = build_parser().parse_args(argv)
    check_args(a)
    from .inference_conditional import load_batch
    from .vae import AutoencoderKLHIP
    from .vae_training import VAEDecoderTrainer, VAETrainer, training_step
    cfg, sd = load_model(a)
    dev = torch.device("cuda", torch.cuda.current_device())
    vae = AutoencoderKLHIP(cfg, device=dev)
    vae.load_state_dict(sd)
    sd = vae.state_dict()                                # (diffusers keys, whatever layout the checkpoint had)
    everything = a.trainable == "all"
    adv = {}
    if a.discriminator:
        if a.discriminator == "metakernel":
            from .metakernel import MetaKernelConfig, MetaKernelDiscriminator
            disc = MetaKernelDiscriminator(MetaKernelConfig(in_channels=cfg.out_channels), seed=a.seed, device=dev, lr=a.lr,
                                           deterministic=a.deterministic)
        else:
            from .discriminator import DiscriminatorConfig, PatchDiscriminator
            disc = PatchDiscriminator(DiscriminatorConfig(in_channels=2 * a.bev_grid[0] if a.disc_bev else cfg.out_channels),
                                      seed=a.seed, device=dev, lr=a.lr, deterministic=a.deterministic)
        if a.disc_state:
            disc.load_state(a.disc_state)
        adv = dict(discriminator=disc, disc_start=a.disc_start, disc_weight=a.disc_weight)
    if a.disc_bev or a.bev_rec_weight > 0:
        adv.update(bev=bev_sensor(cfg.sample_size[1], cfg.sample_size[0], a.bev_grid, a.bev_range), bev_rec_weight=a.bev_rec_weight,
                   disc_bev=a.disc_bev, bev_ordered=a.bev_ordered)
    if everything:
        trainer = VAETrainer(cfg, sd, device=dev, lr=a.lr, kl_weight=a.kl_weight, deterministic=a.deterministic, **adv)
    else:
        trainer = VAEDecoderTrainer(cfg, sd, device=dev, lr=a.lr, deterministic=a.deterministic, **adv)
    shape = (cfg.in_channels, *cfg.sample_size)
    files = sorted(glob.glob(os.path.join(a.input, "*.npy"))) if a.input else None
    if files is not None and not files:
        raise ValueError(f"{a.input}: no .npy range images")
    gen = torch.Generator().manual_seed(a.seed)
    pixels = a.batch_size * shape[1] * shape[2]
    last = None
    for step in range(a.steps):
        if files is not None:
            x = torch.from_numpy(np.stack([np.load(f).astype(np.float32) for f in batch_files(files, step, a.batch_size)]))
            if tuple(x.shape[1:]) != shape:
                raise ValueError(f"range images of shape {tuple(x.shape[1:])}, the VAE expects {shape}")
        else:
            x = load_batch(None, a.batch_size, shape, a.seed)
        if everything:
            loss = trainer.train_step(x.to(dev), sample_posterior=not a.mode, generator=gen)
        else:
            loss = training_step(trainer, vae, x.to(dev), sample_posterior=not a.mode, generator=gen)
        if (step + 1) % a.log_every == 0 or step + 1 == a.steps:
            started = a.discriminator and trainer.last_disc is not None
            last = log_record(step + 1, loss, trainer.last_abs_sums.cpu().tolist(), pixels, trainer.last_kl if everything else None,
                              (trainer.last_g_loss, trainer.last_d_weight, trainer.last_disc) if started else None,
                              trainer.last_bev_rec if a.bev_rec_weight > 0 else None)
            print(json.dumps(last), flush=True)
    trainer.save_pretrained(a.out)
    if a.discriminator:
        trainer.discriminator.save_state(os.path.join(a.out, "discriminator.pt"))
    return last


if __name__ == "__main__":
    main()
    sys.exit(0)
