#!/usr/bin/env python3
"""Throughput of VAE decoder fine-tuning at the shipped config (rangeldm_amd/vae_training.py): samples/s of `training_step` -- frozen
encode + posterior sample on the inference kernels, decoder forward, L1, backward, Adam, operand repack -- batch 8, 1024 x 64, one GPU,
eager launches (no captured step graph exists for this trainer).

    python tools/bench_vae_train.py [--batch 8] [--steps 10] [--warmup 3] [--repeats 5] [--no-unet] [--deterministic]
                                    [--trainable decoder|all] [--discriminator [patchgan|metakernel]] [--disc-bev] [--bev-rec-weight X]
                                    [--bev-ordered]

After the warm-up, --repeats timed runs of --steps steps each (a host clock around work that ends in a device synchronise): median
[min, max].  Achieved TFLOP/s counts 3 x AutoencoderKLHIP.decode_flops (decoder forward + backward; the encode is not counted).  In the
same process the UNet step of tools/bench_train.py (VAE encode + UNet forward / backward / AdamW / EMA from captured step graphs) is
timed the same way, interleaved with the decoder runs, for scale.  --trainable all adds the whole-VAE step (`VAETrainer.train_step`:
encoder, posterior, decoder, L1 + KL, backward through all three, Adam over every parameter; noise drawn on the host as in
`training_step`), interleaved with the other two in the same run (samples/s only: the library counts no encoder FLOPs).  --discriminator
adds the adversarial step of every timed VAE trainer -- a second trainer of the same kind with a PatchDiscriminator and disc_start = 0:
generator term, adaptive weight, mixed backward, the PatchGAN's own hinge step -- interleaved with the plain ones in the same run, and
reports its ratio to the plain step.  --discriminator metakernel times, beside those, the same step against the Meta-Kernel
discriminator (rangeldm_amd/metakernel.py; `vae_decoder_meta` / `vae_all_meta`), all in the same interleaved run.  --disc-bev and / or
--bev-rec-weight X (with --discriminator) time, beside those, the PatchGAN step with the BEV terms of vae_training.py on the KITTI-360
sensor and the reference's [1, 512, 512] volume over +-51.2 m (`vae_decoder_bev` / `vae_all_bev`); with --bev-ordered those trainers
form their volumes with the order-fixed splat (bev_ordered=True) and, under --deterministic, run deterministically like the others
(without it the BEV trainers stay in the default mode: the atomic splat refuses deterministic=True).  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def tri(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-unet", action="store_true", help="skip the UNet step (a profiler run wants the decoder step alone)")
    ap.add_argument("--deterministic", action="store_true", help="VAEDecoderTrainer(deterministic=True)")
    ap.add_argument("--trainable", choices=("decoder", "all"), default="decoder", help="all: also time VAETrainer's whole-VAE step")
    ap.add_argument("--discriminator", nargs="?", const="patchgan", default=None, choices=("patchgan", "metakernel"),
                    help="also time the adversarial step (disc_start = 0) against the PatchGAN; metakernel: and against the Meta-Kernel one")
    ap.add_argument("--disc-bev", action="store_true", help="also time the PatchGAN step on the BEV volume of the reconstruction")
    ap.add_argument("--bev-rec-weight", type=float, default=0.0, metavar="X", help="also time the step with the BEV density L1 term")
    ap.add_argument("--bev-ordered", action="store_true", help="the BEV trainers use the order-fixed splat (and follow --deterministic)")
    ap.add_argument("--seed", type=int, default=20240310)
    a = ap.parse_args()
    if (a.disc_bev or a.bev_rec_weight > 0) and not a.discriminator:
        ap.error("--disc-bev / --bev-rec-weight are timed against the PatchGAN step: pass --discriminator")
    from rangeldm_amd import _lib
    from rangeldm_amd.config import PRESETS
    from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
    from rangeldm_amd.synth import normal, synth_state_dict
    from rangeldm_amd.vae import AutoencoderKLHIP
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer, training_step
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = PRESETS["RangeLDM"]
    cfg = p["vae"]
    sd = synth_state_dict(vae_param_shapes(cfg), seed=a.seed, prefix="vae.")
    vae = AutoencoderKLHIP(cfg)
    vae.load_state_dict(sd)
    tr = VAEDecoderTrainer(cfg, sd, device=dev, deterministic=a.deterministic)
    B = a.batch
    W, H = cfg.sample_size
    n_img = max(a.warmup, a.steps)
    imgs = [torch.from_numpy(normal(a.seed, f"train/0/{i}", (B, cfg.in_channels, W, H))).mul_(0.5).to(dev) for i in range(n_img)]
    gen = torch.Generator().manual_seed(a.seed)
    losses = []

    def vae_steps(n):
        for i in range(n):
            losses.append(training_step(tr, vae, imgs[i], generator=gen))

    all_steps, losses_all = None, []
    if a.trainable == "all":
        tra = VAETrainer(cfg, sd, device=dev, deterministic=a.deterministic)
        agen = torch.Generator().manual_seed(a.seed)

        def all_steps(n):
            for i in range(n):
                losses_all.append(tra.train_step(imgs[i], generator=agen))

    adv_steps, adv_all_steps = None, None
    if a.discriminator:
        from rangeldm_amd.discriminator import PatchDiscriminator
        tr_adv = VAEDecoderTrainer(cfg, sd, device=dev, deterministic=a.deterministic,
                                   discriminator=PatchDiscriminator(seed=a.seed, device=dev, deterministic=a.deterministic))
        ggen = torch.Generator().manual_seed(a.seed)

        def adv_steps(n):
            for i in range(n):
                training_step(tr_adv, vae, imgs[i], generator=ggen)

        if a.trainable == "all":
            tra_adv = VAETrainer(cfg, sd, device=dev, deterministic=a.deterministic,
                                 discriminator=PatchDiscriminator(seed=a.seed, device=dev, deterministic=a.deterministic))
            gagen = torch.Generator().manual_seed(a.seed)

            def adv_all_steps(n):
                for i in range(n):
                    tra_adv.train_step(imgs[i], generator=gagen)

    meta_steps, meta_all_steps = None, None
    if a.discriminator == "metakernel":
        from rangeldm_amd.metakernel import MetaKernelDiscriminator
        tr_meta = VAEDecoderTrainer(cfg, sd, device=dev, deterministic=a.deterministic,
                                    discriminator=MetaKernelDiscriminator(seed=a.seed, device=dev, deterministic=a.deterministic))
        mgen = torch.Generator().manual_seed(a.seed)

        def meta_steps(n):
            for i in range(n):
                training_step(tr_meta, vae, imgs[i], generator=mgen)

        if a.trainable == "all":
            tra_meta = VAETrainer(cfg, sd, device=dev, deterministic=a.deterministic,
                                  discriminator=MetaKernelDiscriminator(seed=a.seed, device=dev, deterministic=a.deterministic))
            magen = torch.Generator().manual_seed(a.seed)

            def meta_all_steps(n):
                for i in range(n):
                    tra_meta.train_step(imgs[i], generator=magen)

    bev_steps, bev_all_steps = None, None
    if a.disc_bev or a.bev_rec_weight > 0:
        from rangeldm_amd.discriminator import PatchDiscriminator
        from rangeldm_amd.range_image import point_cloud_to_range_image_KITTI

        def bev_kw():
            det = bool(a.deterministic and a.bev_ordered)
            return dict(discriminator=PatchDiscriminator(seed=a.seed, device=dev, deterministic=det), deterministic=det,
                        bev_ordered=a.bev_ordered,
                        bev=point_cloud_to_range_image_KITTI(width=W, grid_sizes=[1, 512, 512], pc_range=[-51.2, -51.2, -3., 51.2, 51.2, 1.]),
                        bev_rec_weight=a.bev_rec_weight, disc_bev=a.disc_bev)
        tr_bev = VAEDecoderTrainer(cfg, sd, device=dev, **bev_kw())
        bgen = torch.Generator().manual_seed(a.seed)

        def bev_steps(n):
            for i in range(n):
                training_step(tr_bev, vae, imgs[i], generator=bgen)

        if a.trainable == "all":
            tra_bev = VAETrainer(cfg, sd, device=dev, **bev_kw())
            bagen = torch.Generator().manual_seed(a.seed)

            def bev_all_steps(n):
                for i in range(n):
                    tra_bev.train_step(imgs[i], generator=bagen)

    unet_steps = None
    if not a.no_unet:
        from rangeldm_amd.schedulers import DDPMSchedulerHIP
        from rangeldm_amd.training import UNetTrainer
        from rangeldm_amd.training import training_step as unet_training_step
        utr = UNetTrainer(p["unet"], synth_state_dict(unet_param_shapes(p["unet"]), seed=a.seed), device=dev)
        sched = DDPMSchedulerHIP()
        ugen = torch.Generator().manual_seed(a.seed)

        def unet_steps(n):
            for i in range(n):
                unet_training_step(utr, vae, sched, imgs[i], generator=ugen, pos_encoding=True, graphed=True)

    vae_steps(a.warmup)
    if all_steps is not None:
        all_steps(a.warmup)
    for fn in (adv_steps, adv_all_steps, meta_steps, meta_all_steps, bev_steps, bev_all_steps):
        if fn is not None:
            fn(a.warmup)
    if unet_steps is not None:
        unet_steps(max(a.warmup, 2))                    # (step 1 runs eagerly and sizes the scratch buffers, step 2 captures)
    torch.cuda.synchronize()
    sps = {"vae_decoder": [], "vae_all": [], "unet": [], "vae_decoder_adv": [], "vae_all_adv": [], "vae_decoder_meta": [],
           "vae_all_meta": [], "vae_decoder_bev": [], "vae_all_bev": []}
    for _ in range(a.repeats):
        for name, fn in (("vae_decoder", vae_steps), ("vae_decoder_adv", adv_steps), ("vae_all", all_steps), ("vae_all_adv", adv_all_steps),
                         ("vae_decoder_meta", meta_steps), ("vae_all_meta", meta_all_steps), ("vae_decoder_bev", bev_steps),
                         ("vae_all_bev", bev_all_steps), ("unet", unet_steps)):
            if fn is None:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            sps[name].append(B * a.steps / (time.perf_counter() - t0))
    f = cfg.downscale
    gflop = 3.0 * vae.decode_flops(1, W // f, H // f) / 1e9
    v = tri(sps["vae_decoder"])
    out = {"metric": "VAE decoder fine-tuning samples/sec, shipped config, batch %d, %d x %d, eager" % (B, W, H),
           "unit": "samples/sec", "value": v["median"], "samples_per_sec": v, "ms_per_step": 1e3 * B / v["median"],
           "n_gpus": 1, "batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "deterministic": bool(a.deterministic),
           "gflop_per_sample": gflop, "flop_model": "3 x decode_flops (decoder forward + backward); frozen encode not counted",
           "achieved_tflops": v["median"] * gflop / 1e3, "decoder_parameters": tr.numel,
           "loss_first_last": [float(losses[0]), float(losses[-1])]}
    if all_steps is not None:
        va = tri(sps["vae_all"])
        out["vae_all"] = {"metric": "whole-VAE training samples/sec (encoder + posterior + decoder, L1 + KL), same run", "value": va["median"],
                          "samples_per_sec": va, "ms_per_step": 1e3 * B / va["median"], "parameters": tra.numel,
                          "loss_first_last": [float(losses_all[0]), float(losses_all[-1])]}
    for name, plain in (("vae_decoder_adv", "vae_decoder"), ("vae_all_adv", "vae_all"), ("vae_decoder_meta", "vae_decoder"),
                        ("vae_all_meta", "vae_all"), ("vae_decoder_bev", "vae_decoder"), ("vae_all_bev", "vae_all")):
        if sps[name]:
            t = tri(sps[name])
            kind = "Meta-Kernel" if name.endswith("_meta") else "PatchGAN"
            if name.endswith("_bev"):
                kind = (f"PatchGAN, disc_bev {bool(a.disc_bev)}, bev_rec_weight {a.bev_rec_weight:g}, BEV 512 x 512"
                        f"{', ordered splat' if a.bev_ordered else ''};")
            out[name] = {"metric": f"adversarial step samples/sec ({kind} ndf 64, disc_start 0), same run", "value": t["median"],
                         "samples_per_sec": t, "ms_per_step": 1e3 * B / t["median"],
                         "time_ratio_to_plain": float(np.median(sps[plain]) / t["median"])}
    if unet_steps is not None:
        out["unet_step_samples_per_sec"] = tri(sps["unet"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
