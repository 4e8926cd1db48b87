"""Conditional sampling driver -- the MI355X counterpart of the reference's `ldm/inference_conditional.py` (BASELINE config 4:
`--cfg configs/upsample.yaml`, 16 -> 64 beams; `configs/inpainting.yaml`): LDMUpscalePipelineRange over a fixed batch of
range images, one pass per seed, `densification_{result,target,input}/` or `inpainting_{...}/` next to each other.

    python -m rangeldm_amd.inference_conditional --cfg upsample --samples 32 --out outputs/upsample/generated
    python -m rangeldm_amd.inference_conditional --cfg /path/to/inpainting.yaml --input /data/range_images --weights outputs/inpainting

What is the reference's and what is not:
  * the loop (`ldm/inference_conditional.py:158-210`): ONE batch is taken from the test loader before the loop and re-sampled
    with seed = rank + nproc * i in iteration i; outputs `<j>_seed_<seed>.bin / .png` in the result directory, and for seed 0
    the ground truth and the sparse / masked input in the target / input directories; points farther than 70 m (KITTI-360;
    90 m nuScenes) are dropped; the BEV PNG is the 8-bit density plane.
  * the batch: `--input DIR` reads `*.npy` range images of shape (2, W, H) in the reference's normalisation
    (`point_cloud_to_range_image.normalize`); without it a deterministic synthetic batch stands in (no dataset is reachable
    offline).  `down` / `masked_image` / `inpainting_mask` are derived as `ldm/dataset.py:340-362` does (rangeldm_amd.conditional).
  * the networks: `--weights` = the training run's output_dir (`unet/ vae/ scheduler/`), else synthetic weights.

`--guided` takes an UNCONDITIONAL config (`RangeLDM`, `RangeDM`, or their yaml) instead: the released checkpoints complete a scan by
known-region replacement inside the captured loop (RePaint; rangeldm_amd.schedulers.repaint_program), no conditional UNet needed.

    python -m rangeldm_amd.inference_conditional --guided --cfg RangeLDM --samples 32 --out outputs/guided/generated
    python -m rangeldm_amd.inference_conditional --guided --task densification --cfg RangeDM --jump-length 10 --jump-n-sample 10

The same folders are written (`inpainting_*` / `densification_*`), so `rangeldm_amd.evaluate inpainting | densification` scores them
unchanged.  Densification (every 4th beam known) by latent replacement needs the pixel-space model: no latent pixel is fully known
under that mask.  `--decoder-guidance` densifies (or in-paints) with the LATENT model instead: DDIM with eta = 0 whose clean estimate
is guided through the VAE decoder (rangeldm_amd.guidance), any pixel mask:

    python -m rangeldm_amd.inference_conditional --guided --task densification --cfg RangeLDM --decoder-guidance \
        --guidance-scale 1.0 --guidance-iters 1 --guidance-window 0 1
"""
import argparse
import glob
import os

import numpy as np
import torch

from . import distributed as D
from .conditional import downsample_range_image, inpainting_inputs, sparse_input_image
from .config import PRESETS, UNetConfig, VAEConfig
from .inference import (add_sampling_args, build_models, device_rng_kwargs, make_scheduler, sensor_for, vae_config_for,
                        write_results)


def load_conditional_config(cfg):
    """Preset name ("upsample", "inpainting") or a reference yaml.  The yaml's `upsample` (rate) / `inpainting` (masked
    fraction) select the task; `model_config: null` means the default conditional UNet of ldm/train_conditional.py:232-251
    (latent channels + 8 for up-sampling, + 5 for in-painting)."""
    if cfg in ("upsample", "inpainting"):
        p = dict(PRESETS[cfg])
        p.update(task=cfg, rate=4, fraction=0.0625, steps=50, batch=16, range_limit=70.0)
        return p
    import yaml
    with open(cfg) as f:
        y = yaml.safe_load(f)
    if not y.get("all_circonv", False):
        raise NotImplementedError("only all_circonv configs are supported (ldm/inference_conditional.py:99-114)")
    if not y.get("with_vae", True):
        raise NotImplementedError("the conditional pipelines are latent-space (with_vae)")
    up, inp = y.get("upsample"), y.get("inpainting")
    if bool(up) == bool(inp):
        raise ValueError("exactly one of `upsample` (rate) and `inpainting` (masked fraction) must be set")
    res = tuple(y.get("resolution", (1024, 64)))
    mc = y.get("model_config")
    if mc:
        mc = dict(mc)
        mc["sample_size"] = tuple(mc["sample_size"])
        unet = UNetConfig(**{k: v for k, v in mc.items() if k in UNetConfig.__dataclass_fields__})
    else:
        kw = dict(sample_size=(res[0] // 4, res[1] // 4), in_channels=4 + (8 if up else 5), out_channels=4)
        if y.get("block_out_channels"):
            kw["block_out_channels"] = tuple(y["block_out_channels"])
        unet = UNetConfig(**kw)
    vae = vae_config_for(y, unet, os.path.dirname(os.path.abspath(cfg)))
    return dict(unet=unet, vae=vae, pos_encoding=False, cond_channels=unet.in_channels - unet.out_channels,
                task="upsample" if up else "inpainting", rate=int(up) if up else 0, fraction=float(inp) if inp else 0.0,
                steps=int(y.get("ddpm_num_inference_steps", 50)), batch=int(y.get("eval_batch_size", 16)),
                range_limit=90.0 if y.get("nuscenes") else 70.0)


def load_batch(input_dir, B, shape, seed):
    """(B, 2, W, H) range images: the first B `*.npy` files of `input_dir` (the reference takes one batch of its test loader), or
    a synthetic batch: channel 0 a smooth normalised range profile in [-0.5, 2], channel 1 a remission in [0, 1]."""
    if input_dir:
        files = sorted(glob.glob(os.path.join(input_dir, "*.npy")))[:B]
        if len(files) < B:
            raise ValueError(f"{input_dir}: {len(files)} range images, batch size {B}")
        x = np.stack([np.load(f).astype(np.float32) for f in files])
        if tuple(x.shape[1:]) != tuple(shape):
            raise ValueError(f"range images of shape {x.shape[1:]}, expected {shape}")
        return torch.from_numpy(x)
    from .synth import uniform
    C, W, H = shape
    w = torch.arange(W, dtype=torch.float32)[None, None, :, None] / W
    h = torch.arange(H, dtype=torch.float32)[None, None, None, :] / H
    ph = torch.from_numpy(uniform(seed, "cond/phase", (B, 1, 1, 1)))
    rng = 0.6 + 0.8 * torch.sin(2 * np.pi * (w + ph)) * (0.5 + 0.5 * h) + 0.3 * torch.cos(6 * np.pi * w)
    rem = 0.5 + 0.5 * torch.from_numpy(uniform(seed, "cond/remission", (B, 1, W, H)))
    return torch.cat([rng.expand(B, 1, W, H).clamp(-0.5, 2.0), rem], 1).contiguous()


def guided_known_mask(jpg, task, fraction=0.0625, rate=4):
    """(B, 1, W, H) bool, True = known, and the image shown as the input (-1 where unknown).  inpainting: the reference's mask has
    +1 over the masked azimuth span (conditional.inpainting_inputs), so known = mask < 0; densification: the beams
    downsample_range_image keeps."""
    if task == "inpainting":
        mask, masked = inpainting_inputs(jpg, fraction)
        return mask < 0, masked
    known = torch.zeros((jpg.shape[0], 1, *jpg.shape[2:]), dtype=torch.bool, device=jpg.device)
    known[..., (rate // 2)::rate] = True
    return known, sparse_input_image(jpg, downsample_range_image(jpg, rate), rate)


def main_guided(a):
    """--guided: LDMPipelineRange / DDIMPipelineRange with `known` / `known_mask` on an unconditional config."""
    from .inference import load_config
    from .pipelines import DDIMPipelineRange, LDMPipelineRange
    from .schedulers import DDIMSchedulerHIP

    cfg = load_config(a.cfg)
    if cfg.get("cond_channels", 0):
        raise ValueError(f"--guided takes an unconditional config (RangeLDM, RangeDM); {a.cfg} is conditional")
    guide_kw = {}
    if a.decoder_guidance:
        if cfg["vae"] is None:
            raise ValueError(f"--decoder-guidance guides the latent model through its VAE decoder; {a.cfg} is pixel-space")
        if (a.scheduler or "ddim") != "ddim":
            raise NotImplementedError("--decoder-guidance runs DDIM (eta = 0)")
        if a.jump_length != 1 or a.jump_n_sample != 1:
            raise NotImplementedError("--decoder-guidance does not resample (--jump-length / --jump-n-sample)")
        a.scheduler = "ddim"
        guide_kw = dict(decoder_guidance=True, guidance_scale=a.guidance_scale, guidance_iters=a.guidance_iters,
                        guidance_start=a.guidance_window[0], guidance_stop=a.guidance_window[1])
    if (a.scheduler or "ddpm") in ("dpmsolver++", "unipc"):
        raise NotImplementedError("--guided runs DDPM or DDIM rows (DPM-Solver++ and UniPC keep an x0 history that a jump invalidates)")
    B = a.batch_size or cfg.get("batch", 16)
    steps = a.steps or cfg.get("steps", 50)
    rank, world, local = D.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    out = a.out or os.path.join("outputs", os.path.splitext(os.path.basename(a.cfg))[0], "guided")
    stem = a.task
    result_path, target_path, input_path = (os.path.join(out, f"{stem}_{k}") for k in ("result", "target", "input"))
    for d in (result_path, target_path, input_path):
        os.makedirs(d, exist_ok=True)
    unet, vae, sched_cfg = build_models(cfg, a.weights, a.ema, a.seed)
    if vae is not None:
        pipe = LDMPipelineRange(vae=vae, unet=unet, scheduler=make_scheduler(a.scheduler or "ddpm", sched_cfg, a.solver_order),
                                pos_encoding=cfg["pos_encoding"])
        f = cfg["vae"].downscale
        img_shape = (cfg["vae"].in_channels, cfg["unet"].sample_size[0] * f, cfg["unet"].sample_size[1] * f)
    else:
        pipe = DDIMPipelineRange(unet=unet, scheduler=DDIMSchedulerHIP(sched_cfg), pos_encoding=cfg["pos_encoding"])
        img_shape = (cfg["unet"].out_channels, *cfg["unet"].sample_size)
    jpg = load_batch(a.input, B, img_shape, a.seed).to(dev)
    known_mask, shown = guided_known_mask(jpg, a.task)
    to_range = sensor_for(jpg.shape[3])
    lim = 90.0 if jpg.shape[3] == 32 else 70.0

    n_iter = a.samples // B // world + 1
    for i in range(n_iter):
        seed = rank + world * i
        kw = device_rng_kwargs(a.seed, i, B, rank, world) if a.device_rng else dict(generator=torch.Generator().manual_seed(seed))
        images = pipe(batch_size=B, num_inference_steps=steps, output_type="torch", known=jpg,
                      known_mask=known_mask, jump_length=a.jump_length, jump_n_sample=a.jump_n_sample, **guide_kw, **kw)
        write_results(result_path, to_range, images.contiguous(), seed, lim, a.save_npy)
        if seed == 0:
            write_results(target_path, to_range, jpg, seed, lim, a.save_npy)
            write_results(input_path, to_range, shown.contiguous(), seed, lim, a.save_npy)
    D.barrier()
    if rank == 0:
        print(f"wrote {n_iter * B} guided {stem} results to {result_path}")


def main(argv=None):
    ap = argparse.ArgumentParser(description="RangeLDM conditional sampler on MI355X (ldm/inference_conditional.py counterpart)")
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--input", default=None, help="directory of (2, W, H) .npy range images (default: synthetic batch)")
    ap.add_argument("--weights", default=None, help="reference-style output_dir with unet/ and vae/ safetensors")
    ap.add_argument("--seed", type=int, default=20240310)
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--guided", action="store_true",
                    help="complete the scan with an UNCONDITIONAL config (RangeLDM, RangeDM) by known-region replacement")
    ap.add_argument("--task", choices=("inpainting", "densification"), default="inpainting", help="--guided: which mask")
    ap.add_argument("--jump-length", type=int, default=1, help="--guided: RePaint's jump length (rows re-noised per jump)")
    ap.add_argument("--jump-n-sample", type=int, default=1, help="--guided: RePaint's resampling count (1: no jumps)")
    ap.add_argument("--save-npy", action="store_true", help="--guided: also write the raw (2, W, H) fp32 range images")
    ap.add_argument("--decoder-guidance", action="store_true",
                    help="--guided with a latent config: guide DDIM's clean estimate through the VAE decoder (any mask; densification too)")
    ap.add_argument("--guidance-scale", type=float, default=1.0, help="--decoder-guidance: step length along grad sqrt(L)")
    ap.add_argument("--guidance-iters", type=int, default=1, help="--decoder-guidance: guidance iterations per sampling step")
    ap.add_argument("--guidance-window", type=float, nargs=2, default=(0.0, 1.0), metavar=("A", "B"),
                    help="--decoder-guidance: guide the steps i with A <= i / steps < B")
    add_sampling_args(ap)
    a = ap.parse_args(argv)
    if a.guided:
        return main_guided(a)

    from .encoders import SparseRangeImageEncoder2
    from .pipelines import LDMUpscalePipelineRange

    cfg = load_conditional_config(a.cfg)
    B = a.batch_size or cfg["batch"]
    steps = a.steps or cfg["steps"]
    rank, world, local = D.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    name = os.path.splitext(os.path.basename(a.cfg))[0]
    out = a.out or os.path.join("outputs", name, "generated")
    stem = "densification" if cfg["task"] == "upsample" else "inpainting"
    result_path, target_path, input_path = (os.path.join(out, f"{stem}_{k}") for k in ("result", "target", "input"))
    for d in (result_path, target_path, input_path):
        os.makedirs(d, exist_ok=True)

    unet, vae, sched_cfg = build_models(cfg, a.weights, a.ema, a.seed)
    # ldm/inference_conditional.py:121-134: DDPM scheduler (strided ancestral sampling), SparseRangeImageEncoder2 for up-sampling
    pipe = LDMUpscalePipelineRange(unet=unet, scheduler=make_scheduler(a.scheduler or "ddpm", sched_cfg, a.solver_order), vae=vae)
    condition_encoder = SparseRangeImageEncoder2() if cfg["task"] == "upsample" else None

    f = cfg["vae"].downscale
    img_shape = (cfg["vae"].in_channels, cfg["unet"].sample_size[0] * f, cfg["unet"].sample_size[1] * f)
    jpg = load_batch(a.input, B, img_shape, a.seed).to(dev)
    batch = {"jpg": jpg}
    if cfg["task"] == "upsample":
        batch["down"] = downsample_range_image(jpg, cfg["rate"]).contiguous()
    else:
        batch["inpainting_mask"], batch["masked_image"] = inpainting_inputs(jpg, cfg["fraction"])
    to_range = sensor_for(jpg.shape[3])
    lim = cfg["range_limit"]

    n_iter = a.samples // B // world + 1                   # ldm/inference_conditional.py:158
    for i in range(n_iter):
        seed = rank + world * i
        # :159 (a CPU generator: x_T is drawn on the host, as there)
        kw = device_rng_kwargs(a.seed, i, B, rank, world) if a.device_rng else dict(generator=torch.Generator().manual_seed(seed))
        images = pipe(image=batch["down"] if cfg["task"] == "upsample" else batch["masked_image"],
                      mask=None if cfg["task"] == "upsample" else batch["inpainting_mask"],
                      condition_encoder=condition_encoder, batch_size=B,
                      num_inference_steps=steps, output_type="torch", **kw)
        write_results(result_path, to_range, images, seed, lim)
        if seed == 0:                                      # :196-210
            write_results(target_path, to_range, jpg, seed, lim)
            shown = (sparse_input_image(jpg, batch["down"], cfg["rate"]) if cfg["task"] == "upsample"
                     else batch["masked_image"])
            write_results(input_path, to_range, shown.contiguous(), seed, lim)
    D.barrier()
    if rank == 0:
        print(f"wrote {n_iter * B} {stem} results to {result_path}")


if __name__ == "__main__":
    main()
