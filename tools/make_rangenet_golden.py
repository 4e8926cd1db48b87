#!/usr/bin/env python3
"""Write tests/golden/rangenet.npz: what the reference's RangeNet++ computes, recorded on CPU fp32.

    python tools/make_rangenet_golden.py --reference /path/to/RangeLDM [--out tests/golden/rangenet.npz]

The reference's own modules do the computing: backbones/darknet.py and tasks/semantic/decoders/darknet.py are loaded by path
(modules/segmentator.py needs the `imp` module Python no longer ships, so the head is composed here as segmentator.py:47-50
does: Dropout2d, Conv2d(32, 20, 3, padding=1)), rangeldm_amd.rangenet.synthetic_state is loaded into them with strict=True,
and they run in eval mode.  The activation is read back from the `.npy` the reference's Decoder.forward itself writes into a
temporary frd_dir.  The projection cases come from the reference's LaserScan (modules/kittiparser.py) and the normalisation of
kittiparser.py:391-395; the segmentation cases from sklearn.metrics.jaccard_score(average="weighted"), what metrics/metrics/iou.py
calls.  Only arrays are written.

Keys
  seed, head_bias_std                 the synthetic network: rangenet.synthetic_state(arch, seed, stats, head_bias_std).  The spread of
                                      the head's class biases is the smallest of HEAD_BIAS_STDS at which the full-size case's top-2
                                      margin exceeds 4 x full_emul_logit_err at 90 % of the pixels or more (chosen and verified with
                                      the emulation alone).  The head's weight scale cannot do that: it scales margin and rounding
                                      noise alike (38.6 % of the pixels at any scale); class priors, which a real network's head has
                                      too, widen the margin and leave the noise alone
  bn{21,53}_mean / _var               BatchNorm running statistics of every layer in walk order, fp16 (the state uses the fp16
                                      values): one calibration pass of forward_host over the full-size scan below, so that every
                                      layer's output RMS stays within [0.1, 10]
  small{21,53}_x / _feat / _logits    B = 2, 8 x 64 crops of two other seeded scans; the decoder's output and the head's
  full_input_crc                      crc32 of project_scan(synthetic_cloud(FULL_SEED)): the full-size DarkNet53 input
  full_gathered                       the 4 096 metrics.frd_indices() values of its (1, 32, 64, 1024) activation
  full_argmax, full_margin            per pixel: the argmax and the top-2 logit margin (fp16, rounded towards zero)
  full_emul_rel_l2, full_emul_logit_err   forward_host(bf16=True) against the reference: rel-L2 on the gathered values, max-abs
                                      on the logits -- the rounding the design accepts, never measured on the kernel
  proj{0,1}_points / _remission / _out / _mask   LaserScan + normalisation of two seeded clouds with pairwise distinct depths
  seg_cases, seg{i}_pred / _target / _iou / _accuracy
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rangeldm_amd import rangenet as R                   # noqa: E402
from rangeldm_amd import synth                           # noqa: E402
from rangeldm_amd.metrics import frd_indices             # noqa: E402

TRAIN = "metrics/rangenetpp/lidar_bonnetal_master/train"
FULL_SEED = 53                                           # tests/test_rangenet_host.py: FULL_SEED
HEAD_BIAS_STDS = (0.02, 2.0, 4.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0)


def load_module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Reference:
    def __init__(self, root, arch, sds):
        bb = load_module(os.path.join(root, TRAIN, "backbones/darknet.py"), "ref_backbone")
        dec = load_module(os.path.join(root, TRAIN, "tasks/semantic/decoders/darknet.py"), "ref_decoder")
        self.backbone = bb.Backbone(params=arch["backbone"])
        self.decoder = dec.Decoder(params=arch["decoder"], stub_skips=None, OS=arch["backbone"]["OS"],
                                   feature_depth=self.backbone.get_last_depth())
        self.head = torch.nn.Sequential(torch.nn.Dropout2d(p=arch["head"]["dropout"]),
                                        torch.nn.Conv2d(self.decoder.get_last_depth(), R.NUM_CLASSES, kernel_size=3, stride=1, padding=1))
        for mod, sd in zip((self.backbone, self.decoder, self.head), sds):
            mod.load_state_dict(sd, strict=True)
            mod.eval()

    @torch.no_grad()
    def __call__(self, x):
        """(the dumped activation (B, 32, H, W), logits): segmentator.py:149-153 up to the softmax"""
        with tempfile.TemporaryDirectory() as frd_dir:
            y, skips = self.backbone(x)
            y = self.decoder(y, skips, frd_dir)
            feat = torch.from_numpy(np.load(os.path.join(frd_dir, f"{self.decoder.index - 1}.npy")))
            return feat, self.head(y)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rangenet.npz"))
    a = ap.parse_args()
    seed = synth.DEFAULT_SEED
    out = {"seed": np.int64(seed)}

    pts, rem = R.synthetic_cloud(FULL_SEED)
    full, _ = R.project_scan(pts, rem)
    full_x = torch.from_numpy(full)[None]
    out["full_input_crc"] = np.int64(zlib.crc32(full.tobytes()))
    crops = []
    for s, (r0, c0) in ((21, (20, 300)), (22, (40, 700))):
        p, _ = R.project_scan(*R.synthetic_cloud(s))
        crops.append(p[:, r0:r0 + 8, c0:c0 + 64])
    small_x = torch.from_numpy(np.stack(crops))

    stats = {}
    for layers in (21, 53):
        arch = R.synthetic_arch(layers)
        cal = []
        R.forward_host(R.fold_state(arch, *R.synthetic_state(arch, seed)), full_x, calibrate=cal)
        mean = np.concatenate([m.numpy() for m, _ in cal]).astype(np.float16)
        var = np.concatenate([v.numpy() for _, v in cal]).astype(np.float16)
        assert np.isfinite(mean.astype(np.float32)).all() and (var.astype(np.float32) > 0).all() and np.isfinite(var.astype(np.float32)).all()
        out[f"bn{layers}_mean"], out[f"bn{layers}_var"] = mean, var
        stats[layers] = R.bn_stats_from_arrays(layers, mean, var)

    # the head's bias spread: the smallest candidate whose margins are wide enough, judged by the emulation against fp32
    # forward_host (the reference's run below then records the figures the test uses, and asserts the 90 % again)
    arch53 = R.synthetic_arch(53)
    bias_std = None
    for cand in HEAD_BIAS_STDS:
        st = R.fold_state(arch53, *R.synthetic_state(arch53, seed, stats[53], head_bias_std=cand))
        if bias_std is None:
            (_, l32), (_, l16) = R.forward_host(st, full_x), R.forward_host(st, full_x, bf16=True)
            base = l32 - st["specs"][-1]["shift"].view(1, -1, 1, 1)              # the logits without the bias
            err = float((l16 - l32).abs().max())
        top2 = torch.topk(base[0] + st["specs"][-1]["shift"].view(-1, 1, 1), 2, dim=0).values
        share = float(((top2[0] - top2[1]) > 4 * err).float().mean())
        print(f"head bias std {cand}: margin > 4 x {err:.3f} at {share:.1%} of the pixels")
        bias_std = cand
        if share >= 0.91:
            break
    out["head_bias_std"] = np.float64(bias_std)

    refs = {}
    for layers in (21, 53):
        arch = R.synthetic_arch(layers)
        sds = R.synthetic_state(arch, seed, stats[layers], head_bias_std=bias_std)
        state = R.fold_state(arch, *sds)
        ref = refs[layers] = (Reference(a.reference, arch, sds), state)
        feat, logits = ref[0](small_x)
        out[f"small{layers}_x"], out[f"small{layers}_feat"], out[f"small{layers}_logits"] = small_x.numpy(), feat.numpy(), logits.numpy()
        f, l, rms = R.forward_host(state, small_x, return_rms=True)
        fe, le = R.forward_host(state, small_x, bf16=True)
        print(f"DarkNet{layers} small: forward_host rel-L2 {rel_l2(f, feat):.2e} / {rel_l2(l, logits):.2e}, emulation "
              f"{rel_l2(fe, feat):.2e} / {rel_l2(le, logits):.2e}, layer RMS in [{min(rms):.3f}, {max(rms):.3f}]")
        assert 0.1 <= min(rms) and max(rms) <= 10.0

    ref, state = refs[53]
    feat, logits = ref(full_x)
    idx = np.asarray(frd_indices(), dtype=np.int64)
    gathered = feat.reshape(-1)[idx]
    top2 = torch.topk(logits[0], 2, dim=0).values
    margin = (top2[0] - top2[1]).numpy()
    m16 = margin.astype(np.float16)
    m16 = np.where(m16.astype(np.float32) > margin, np.nextafter(m16, np.float16(0)), m16)      # never above the fp32 margin
    fe, le = R.forward_host(state, full_x, bf16=True)
    e_feat, e_logit = rel_l2(fe.reshape(-1)[idx], gathered), float((le - logits).abs().max())
    confident = m16.astype(np.float32) > 4 * e_logit
    agree = (le[0].argmax(0) == logits[0].argmax(0)).numpy()
    print(f"full size: emulation rel-L2 {e_feat:.3e} on the gathered features ({rel_l2(fe, feat):.3e} on all), max-abs logit error "
          f"{e_logit:.3e}; margin > 4 x that at {confident.mean():.1%} of the pixels; the emulation's argmax agrees at "
          f"{agree.mean():.2%} of all and {agree[confident].mean():.2%} of those; logits RMS {float(logits.pow(2).mean().sqrt()):.3f}")
    assert confident.mean() >= 0.9
    out.update(full_gathered=gathered.numpy().astype(np.float32), full_argmax=logits[0].argmax(0).numpy().astype(np.uint8),
               full_margin=m16, full_emul_rel_l2=np.float64(e_feat), full_emul_logit_err=np.float64(e_logit))

    kp = load_module(os.path.join(a.reference, TRAIN, "tasks/semantic/modules/kittiparser.py"), "ref_kittiparser")
    for i, (s, n, hw, with_rem) in enumerate(((31, 4000, (16, 128), True), (32, 1500, (8, 64), False))):
        pts, rem = R.synthetic_cloud(s, n=n)
        scan = kp.LaserScan(project=True, H=hw[0], W=hw[1], fov_up=3.0, fov_down=-25.0)
        scan.set_points(pts, rem if with_rem else None)
        proj = torch.cat([torch.from_numpy(scan.proj_range).unsqueeze(0).clone(), torch.from_numpy(scan.proj_xyz).clone().permute(2, 0, 1),
                          torch.from_numpy(scan.proj_remission).unsqueeze(0).clone()])
        proj = (proj - torch.tensor(R.IMG_MEANS, dtype=torch.float)[:, None, None]) / torch.tensor(R.IMG_STDS, dtype=torch.float)[:, None, None]
        proj = proj * torch.from_numpy(scan.proj_mask).float()
        out.update({f"proj{i}_points": pts, f"proj{i}_remission": rem, f"proj{i}_out": proj.numpy(), f"proj{i}_mask": scan.proj_mask})

    from sklearn.metrics import jaccard_score
    rng = np.random.default_rng(5)
    cases = []
    t = rng.integers(0, 20, (2, 16, 64))
    cases.append((np.where(rng.random(t.shape) < 0.7, t, rng.integers(0, 20, t.shape)), t))       # every class, 70 % agreement
    t = rng.choice([0, 3, 9], (1, 8, 32))
    cases.append((np.where(rng.random(t.shape) < 0.5, t, rng.choice([3, 9, 11], t.shape)), t))    # a class only the prediction holds
    t = rng.integers(0, 20, (1, 4, 16))
    cases.append((t.copy(), t))                                                                     # identical
    cases.append((np.full((1, 4, 16), 7), rng.choice([7, 8], (1, 4, 16))))                          # a constant prediction
    out["seg_cases"] = np.int64(len(cases))
    for i, (p, t) in enumerate(cases):
        out.update({f"seg{i}_pred": p.astype(np.int64), f"seg{i}_target": t.astype(np.int64),
                    f"seg{i}_iou": np.float64(jaccard_score(t.reshape(-1), p.reshape(-1), average="weighted")),
                    f"seg{i}_accuracy": np.float64((t == p).sum() / float(t.size))})
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
