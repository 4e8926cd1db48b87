"""Evaluation on the MI355X: score what the VAE and the conditional sampler reconstruct, and what the sampler generates.

    python -m rangeldm_amd.evaluate vae --weights outputs/RangeLDM --samples 1000 --batch-size 4 [--input DIR] [--voxel 0.1]
                                        [--match TAU [TAU ...]] [--dcd-alpha A] [--normals K]
    python -m rangeldm_amd.evaluate densification --exp outputs/upsample/generated [--cfg upsample] [--voxel 0.1] [--match ..] [--dcd-alpha A] [--normals K]
    python -m rangeldm_amd.evaluate inpainting --exp outputs/inpainting/generated [--cfg inpainting] [--voxel 0.1] [--match ..] [--dcd-alpha A] [--normals K]
    python -m rangeldm_amd.evaluate chamfer A_DIR B_DIR [--voxel 0.1] [--match TAU [TAU ...]] [--dcd-alpha A] [--normals K]
    python -m rangeldm_amd.evaluate generation GEN_DIR REF_DIR [--points 2048] [--limit N] [--seed 0] [--max-depth M]
                                               [--sampling {random,fps}] [--emd [--emd-eps 0.0078125]]
    python -m rangeldm_amd.evaluate frd FOLDER1 FOLDER2 [--limit 1100] [--rangenet MODEL_DIR [--projection {host,device}]]
    python -m rangeldm_amd.evaluate features GEN_DIR REF_DIR [--k 5] [--limit N] [--subset-size M --subsets S --seed 0]
                                             [--total T --count C] [--rangenet MODEL_DIR [--projection {host,device}]]
    python -m rangeldm_amd.evaluate rangenet --model MODEL_DIR --dump CLOUD_DIR --frd-dir OUT_A --output-dir OUT_S
                                             [--projection {host,device}] [--labels-dir OUT_L [--knn]]
    python -m rangeldm_amd.evaluate segmentation RESULT_SEG_DIR TARGET_SEG_DIR

Every command prints one JSON object on stdout (`--json PATH` also writes it).  Under `torch.distributed.run` the work is
sharded over the ranks and rank 0 reduces and prints.  The arithmetic runs in librangeldm_hip (rangeldm_amd/csrc/chamfer.hip
and lidar.hip); Chamfer distance (CD) is pytorch3d.loss.chamfer_distance's default: per pair
mean_x min_y |x - y|^2 + mean_y min_x |x - y|^2 over xyz.

  vae            ldm/convert_vae.py:221-271: the round trip `vae(batch).sample` over the test range images (`--input DIR` of
                 (2, W, H) .npy files, else the synthetic batch of inference_conditional.load_batch); MAE and PSNR per image
                 on channel 0 mapped to (x * std + mean) / range_fill_value[0] and channel 1 as is, averaged over images;
                 CD between filter_points(to_pc_torch(.), 70) of input and reconstruction.
  densification  metrics/metrics/mae.py:45-89 (`metric.py --mae`) on the layout inference_conditional writes: result
                 `<j>_seed_<s>.bin` against target `<j>_seed_0.bin`, both re-projected with the KITTI sensor's project();
                 range MAE in metres over all W x H pixels and CD, for ours and the nearest / bicubic beam-upsampling
                 baselines built from every `rate`-th beam of the target.
  inpainting     mae.py:91-117 (`metric.py --inpainting_mae`): range MAE in metres over the config's masked azimuth span,
                 with the reference's denominator (files x W x H, mae.py:111) and per masked pixel; and CD.
  chamfer        mean CD over the .bin files of two folders, paired by name (A_DIR the results, B_DIR the targets).
  --voxel SIZE   (vae, densification, inpainting, chamfer) adds the voxel-occupancy scores of the up-sampling and completion
                 tables (Implicit LiDAR Network, TULIP: SIZE 0.1) over the clouds the CD is taken on, through
                 metrics.voxel_scores (rangeldm_amd/csrc/voxel.hip): both clouds of a pair are quantised to floor(c / SIZE)
                 in fp32, a / b / c = the distinct voxels of the result / of the target / of both.  The object gains
                 "voxel": SIZE and "occupancy": the means over pairs of iou = c / (a + b - c), precision = c / a,
                 recall = c / b, f1 = 2c / (a + b), and the integer totals over pairs voxels_result, voxels_target,
                 voxels_both (the same for any number of ranks).  Precision is about the result: for `vae` the result is
                 the reconstruction, for `chamfer` A_DIR; `densification` gives one block per method, like "cd".
                 Without the flag the object is what it was.
  --match TAU [TAU ...]   (the same four commands, the same clouds and the same result / target roles as --voxel) adds the
                 F-score at each distance threshold TAU in metres: "match": {"tau", "precision", "recall", "fscore"}, each a
                 list with one entry per TAU, the means over pairs of precision = the share of result points within TAU of the
                 target, recall = the share of target points within TAU of the result, fscore = 2pr / (p + r) (0 when both
                 are 0); and in the same block the integer totals over pairs matched_result, matched_target (per TAU),
                 points_result, points_target.  It also adds "hausdorff": {"mean", "max"} over the pairs' symmetric Hausdorff
                 distances (the worst point of a pair, which the mean CD hides).
  --dcd-alpha A  (the same commands) adds "dcd": {"alpha": A, "mean"}: the density-aware Chamfer distance of
                 metrics.density_aware_chamfer (squared distance in the exponent, no size-ratio factor), the mean over pairs.
                 With either flag a batch of pairs goes through ONE nearest-neighbour search, metrics.pair_scores
                 (rangeldm_amd/csrc/nn_index.hip), and "cd" is taken from that search's distances: they are the bits the plain
                 search gives and go through the same means, so "cd" is unchanged.  Without the flags the object is what
                 it was.
  --normals K    (the same commands, the same clouds and roles) adds "plane": {"k": K, "cd_plane", "normal_consistency"}, the
                 means over pairs of metrics.plane_scores (rangeldm_amd/csrc/knn.hip): surface normals by PCA over the K
                 nearest neighbours of each cloud (1 <= K <= 32), the point-to-plane Chamfer distance (the squared distance
                 to the tangent plane at the nearest point of the other cloud, both directions added) and pytorch3d's normal
                 consistency.  A pair's values depend on the pair alone, so the block is the same for any number of ranks.
                 Without the flag the object is what it was.
  generation     set-level metrics of a folder of generated .bin clouds against a folder of reference sweeps (Achlioptas et
                 al. 2018; Yang et al. 2019): MMD-CD, COV-CD and 1-NNA-CD (metrics.set_metrics) from the all-pairs Chamfer
                 matrices, every cloud cut to the points closer than --max-depth and sub-sampled to --points
                 (metrics.subsample with seed + file index; --sampling fps: by farthest point sampling, the protocol's
                 choice, metrics.farthest_point_sample, and the object then carries "sampling": "fps"); the BEV-histogram jsd / mmd of metrics.evaluate_folders on the
                 full clouds beside them.  Each rank computes a block of rows of each matrix; an entry does not depend on the
                 block it was computed in, so the result is the same for any number of ranks.  --emd adds MMD-EMD, COV-EMD
                 and 1-NNA-EMD from the all-pairs Earth Mover's Distance matrices (metrics.emd_matrix: an auction that ends
                 at --emd-eps metres); EMD is a one-to-one matching, so every cloud must then hold exactly --points points
                 (at most 2 048) after the depth cut.
  frd            `metric.py --fid --fid_folder1 FOLDER1 --fid_folder2 FOLDER2` (metrics/metrics/fid/lidargen_fid.py get_fid): the
                 Frechet distance between two folders of dumped RangeNet++ activations (`.npy`, 2 097 152 values each), on
                 the reference's 4 096 randomly drawn values per file and at most --limit files per folder (sorted by name),
                 by metrics.frechet_distance.  The work is one small matrix: rank 0 alone loads and computes, so the output
                 is the same for any number of ranks.  With --rangenet MODEL_DIR the two folders hold point clouds (`.bin`,
                 x y z remission) instead: every cloud (sorted by name, at most --limit) is projected and run through
                 RangeNet++ (rangenet.RangeNet), shared out over the ranks, and only its 4 096 drawn values are kept -- the
                 same numbers, bit for bit, as `rangenet` dumps and a plain `frd` of the dumped folders then reads.
                 --projection device projects a chunk of clouds in one call on the GPU (rangenet.project_scans) instead of one
                 by one in numpy; the object then carries "projection": "device".  The device's atan2 / asin are not
                 numpy's, so a point within a few ulp of a pixel boundary may land next door: the two projections agree with
                 themselves (`rangenet --projection device` dumps what `frd --rangenet --projection device` draws from), not
                 bit for bit with each other.
  features       what the Frechet distance leaves open, over the same inputs `frd` reads (two folders of dumped activations, or
                 with --rangenet two folders of clouds; every file, sorted by name, unless --limit): the kernel distance krd
                 (metrics.kernel_distance: KID's unbiased polynomial-kernel MMD^2, which has no bias that depends on the
                 number of files; --subset-size M gives the mean krd and krd_std over --subsets draws of M rows per set) and
                 precision / recall / density / coverage of GEN_DIR against REF_DIR on --k nearest-neighbour manifolds
                 (metrics.prdc: Kynkaanniemi et al. 2019, Naeem et al. 2020).  Row scans on the fp64 MFMA, no n x n matrix.
                 As in `frd` the forwards are shared out over the ranks and rank 0 goes on alone.
  rangenet       `rangenetpp.main(... --dump CLOUD_DIR --frd_dir OUT_A --output_dir OUT_S --point_cloud)` (metric.py's feature
                 dump; tasks/semantic/infer_lib.py, modules/user.py:130-184): the i-th `.bin` cloud of CLOUD_DIR IN SORTED
                 ORDER (the reference takes glob order, which is arbitrary) gives OUT_A/i.npy, the decoder's last feature map
                 (1, 32, 64, 1024) float32, and OUT_S/i.pth, the (64, 1024) int64 argmax tensor (torch.save).  Cloud i is the
                 work of rank i mod world.  MODEL_DIR is laid out like the reference's darknet53-1024/.
                 --labels-dir OUT_L (with --projection device) also writes OUT_L/i.label, one uint32 per point of cloud i
                 (SemanticKITTI's format): the argmax of the point's pixel (user.py's `proj_argmax[p_y, p_x]`), or with
                 --knn the vote of postproc/KNN.py with the `post.KNN.params` of MODEL_DIR/arch_cfg.yaml; mapped through
                 `learning_map_inv` of MODEL_DIR/data_cfg.yaml when that file exists (the reference's to_original), else
                 the network's class ids.
  segmentation   `metric.py --iou / --accuracy` (metrics/metrics/iou.py): the `.pth` label tensors of two folders, paired by name,
                 compared through one 20 x 20 confusion matrix counted on the device: accuracy, and
                 jaccard_score(target, result, average="weighted").

Only the linear range normalisation (x * std + mean, every shipped config) is supported: `log` / `inverse` sensors raise
NotImplementedError.  nuScenes `.bin` files carry no ring column, so they cannot be re-projected: nuScenes raises too.
"""
import argparse
import glob
import json
import math
import os
import re

import numpy as np
import torch

from . import distributed as D

_RESULT_RE = re.compile(r"^(\d+)_seed_(\d+)\.bin$")


# ---- host-side helpers (no GPU) ---------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m rangeldm_amd.evaluate",
                                 description="reconstruction metrics (MAE, PSNR, Chamfer distance, voxel occupancy, F-score, Hausdorff, DCD) and set-level generation "
                                             "metrics (MMD-CD, COV-CD, 1-NNA-CD) on MI355X")
    sub = ap.add_subparsers(dest="cmd", required=True)

    v = sub.add_parser("vae", help="VAE round trip: MAE, PSNR, CD (ldm/convert_vae.py:193-271)")
    v.add_argument("--weights", default=None, help="diffusers VAE directory, or a training output_dir holding vae/")
    v.add_argument("--sgm-ckpt", default=None, help="sgm AutoencodingEngine .ckpt (ldm/convert_vae.py:149-189)")
    v.add_argument("--sgm-yaml", default=None, help="the yaml the sgm checkpoint was trained with")
    v.add_argument("--input", default=None, help="directory of (2, W, H) .npy range images (default: synthetic batch)")
    v.add_argument("--samples", type=int, default=1000)
    v.add_argument("--batch-size", type=int, default=4)
    v.add_argument("--seed", type=int, default=20240310)
    voxel_help = ("also report voxel-occupancy IoU / precision / recall / F1 of result against target on a grid of SIZE metres "
                  "(0.1 in the up-sampling literature)")
    match_help = ("also report precision / recall / F-score of result against target at each distance threshold TAU (metres), "
                  "and the Hausdorff distance")
    normals_help = ("also report the point-to-plane Chamfer distance and the normal consistency, with PCA normals over the K nearest "
                    "neighbours (1..32)")
    dcd_help = "also report the density-aware Chamfer distance (Wu et al. 2021) with this alpha (per square metre; no default)"

    for task in ("densification", "inpainting"):
        t = sub.add_parser(task, help=f"{task} results of inference_conditional against their targets")
        t.add_argument("--exp", required=True, help=f"directory holding {task}_result/ and {task}_target/")
        t.add_argument("--cfg", default="upsample" if task == "densification" else "inpainting",
                       help="preset name or reference yaml (rate / masked fraction, sensor)")
        t.add_argument("--voxel", type=float, default=None, metavar="SIZE", help=voxel_help)
        t.add_argument("--match", type=float, nargs="+", default=None, metavar="TAU", help=match_help)
        t.add_argument("--dcd-alpha", type=float, default=None, metavar="A", help=dcd_help)
        t.add_argument("--normals", type=int, default=None, metavar="K", help=normals_help)

    c = sub.add_parser("chamfer", help="mean CD over .bin files of two folders, paired by name")
    c.add_argument("a_dir")
    c.add_argument("b_dir")
    c.add_argument("--columns", type=int, default=4, help="float32 columns per point in the .bin files")
    for p in (v, c):
        p.add_argument("--voxel", type=float, default=None, metavar="SIZE", help=voxel_help)
        p.add_argument("--match", type=float, nargs="+", default=None, metavar="TAU", help=match_help)
        p.add_argument("--dcd-alpha", type=float, default=None, metavar="A", help=dcd_help)
        p.add_argument("--normals", type=int, default=None, metavar="K", help=normals_help)

    g = sub.add_parser("generation", help="MMD-CD / COV-CD / 1-NNA-CD (+ BEV jsd / mmd) of generated against reference clouds")
    g.add_argument("gen_dir")
    g.add_argument("ref_dir")
    g.add_argument("--points", type=int, default=2048, help="points kept per cloud (deterministic sub-sample)")
    g.add_argument("--limit", type=int, default=None, help="use the first N files (sorted by name) of each folder")
    g.add_argument("--seed", type=int, default=0, help="sub-sampling seed (file i uses seed + i)")
    g.add_argument("--max-depth", type=float, default=None, help="drop points at this distance from the sensor or farther")
    g.add_argument("--sampling", choices=("random", "fps"), default="random",
                   help="how a cloud is cut to --points: a uniform random draw, or farthest point sampling (started at a "
                        "seeded random point)")
    g.add_argument("--columns", type=int, default=4, choices=(4, 5),
                   help="float32 columns per point of the REFERENCE files (5: nuScenes sweeps); generated files have 4")
    g.add_argument("--emd", action="store_true",
                   help="also MMD-EMD / COV-EMD / 1-NNA-EMD (every cloud must hold --points points, at most 2048)")
    g.add_argument("--emd-eps", type=float, default=2.0 ** -7,
                   help="final epsilon of the EMD auction, metres: the matching cost is within about this of the optimum")

    f = sub.add_parser("frd", help="Frechet distance between two folders of dumped activations (metric.py --fid)")
    f.add_argument("folder1")
    f.add_argument("folder2")
    f.add_argument("--limit", type=int, default=1100, help="use the first N files (sorted by name) of each folder")
    f.add_argument("--total", type=int, default=2097152, help="values per dumped file (other than the default: tests)")
    f.add_argument("--count", type=int, default=4096, help="values drawn per file (other than the default: tests)")

    f.add_argument("--rangenet", default=None, metavar="MODEL_DIR",
                   help="the folders hold .bin point clouds: run RangeNet++ from this model folder over them first")
    f.add_argument("--projection", choices=("host", "device"), default="host",
                   help="with --rangenet: project the clouds one by one in numpy, or a chunk at a time on the GPU")

    ft = sub.add_parser("features", help="kernel distance and precision / recall / density / coverage over the activations frd reads")
    ft.add_argument("gen_dir")
    ft.add_argument("ref_dir")
    ft.add_argument("--k", type=int, default=5, help="neighbours of the manifolds' radii")
    ft.add_argument("--limit", type=int, default=None, help="use the first N files (sorted by name) of each folder; default: all")
    ft.add_argument("--subset-size", type=int, default=None, help="rows per set of one kernel-distance estimate; default: the full sets, once")
    ft.add_argument("--subsets", type=int, default=100, help="with --subset-size: estimates the mean and deviation are taken over")
    ft.add_argument("--seed", type=int, default=0, help="with --subset-size: seed of the row draws")
    ft.add_argument("--total", type=int, default=2097152, help="values per dumped file (other than the default: tests)")
    ft.add_argument("--count", type=int, default=4096, help="values drawn per file (other than the default: tests)")
    ft.add_argument("--rangenet", default=None, metavar="MODEL_DIR",
                   help="the folders hold .bin point clouds: run RangeNet++ from this model folder over them first")
    ft.add_argument("--projection", choices=("host", "device"), default="host",
                   help="with --rangenet: project the clouds one by one in numpy, or a chunk at a time on the GPU")

    r = sub.add_parser("rangenet", help="RangeNet++ over a folder of clouds: FRD activations and segmentations (rangenetpp --dump)")
    r.add_argument("--model", required=True, help="model folder: arch_cfg.yaml, backbone, segmentation_decoder, segmentation_head")
    r.add_argument("--dump", required=True, help="folder of .bin point clouds (x y z remission, float32)")
    r.add_argument("--frd-dir", required=True, help="where i.npy, the (1, 32, 64, 1024) activation of cloud i, is written")
    r.add_argument("--output-dir", required=True, help="where i.pth, the argmax tensor of cloud i, is written")
    r.add_argument("--batch-size", type=int, default=4)
    r.add_argument("--projection", choices=("host", "device"), default="host",
                   help="project the clouds one by one in numpy, or a chunk at a time on the GPU")
    r.add_argument("--labels-dir", default=None,
                   help="where i.label, one uint32 label per point of cloud i, is written (needs --projection device)")
    r.add_argument("--knn", action="store_true",
                   help="with --labels-dir: clean the labels with the KNN vote of the model's post.KNN.params")

    s = sub.add_parser("segmentation", help="IoU (weighted Jaccard) and accuracy of two folders of .pth label tensors")
    s.add_argument("result_dir")
    s.add_argument("target_dir")
    s.add_argument("--classes", type=int, default=20)

    for p in (v, *[sub.choices[k] for k in ("densification", "inpainting")], c, g, f, ft, r, s):
        p.add_argument("--json", default=None, help="also write the result object to this file")
    return ap


def pair_result_files(result_dir, target_dir):
    """[(result_path, target_path)] sorted by (j, seed): every `<j>_seed_<s>.bin` of result_dir with `<j>_seed_0.bin` of
    target_dir (inference_conditional writes the target once, for seed 0).  A result without its target is an error."""
    found = []
    for path in glob.glob(os.path.join(result_dir, "*.bin")):
        m = _RESULT_RE.match(os.path.basename(path))
        if m:
            found.append((int(m.group(1)), int(m.group(2)), path))
    pairs = []
    for j, s, path in sorted(found):
        target = os.path.join(target_dir, f"{j}_seed_0.bin")
        if not os.path.isfile(target):
            raise FileNotFoundError(f"{path}: no target {target}")
        pairs.append((path, target))
    if not pairs:
        raise FileNotFoundError(f"no <j>_seed_<s>.bin results in {result_dir}")
    return pairs


def pair_by_name(a_dir, b_dir):
    """[(a_path, b_path)] for the .bin names present in both folders, sorted by name."""
    a = {os.path.basename(p) for p in glob.glob(os.path.join(a_dir, "*.bin"))}
    b = {os.path.basename(p) for p in glob.glob(os.path.join(b_dir, "*.bin"))}
    common = sorted(a & b)
    if not common:
        raise FileNotFoundError(f"no .bin file name common to {a_dir} and {b_dir}")
    return [(os.path.join(a_dir, n), os.path.join(b_dir, n)) for n in common]


def range_affine(sensor):
    """(std, mean) of the sensor's range normalisation: metres = x * std + mean.  Only the linear map is supported."""
    if getattr(sensor, "log", False) or getattr(sensor, "inverse", False):
        raise NotImplementedError("range MAE in metres is implemented for the linear normalisation only "
                                  "(log / inverse sensors are not)")
    return float(sensor.std), float(sensor.mean)


def require_reprojectable(sensor):
    """The .bin protocol re-projects returns with the sensor's project(): KITTI-360 finds the beam from the inclination;
    nuScenes needs the ring column, which the written (x, y, z, remission) files do not carry."""
    from .range_image import point_cloud_to_range_image_nuScenes
    if isinstance(sensor, point_cloud_to_range_image_nuScenes):
        raise NotImplementedError("nuScenes .bin files carry no ring column: they cannot be re-projected")
    return sensor


def task_sensor(cfg_arg):
    """The sensor a conditional config's images come from, with the yaml's `log` / `inverse` switches."""
    from .inference import sensor_for
    from .inference_conditional import load_conditional_config
    cfg = load_conditional_config(cfg_arg)
    kw = {}
    if cfg_arg not in ("upsample", "inpainting"):
        import yaml
        with open(cfg_arg) as f:
            y = yaml.safe_load(f)
        kw = {k: bool(y[k]) for k in ("log", "inverse") if k in y}
    beams = cfg["unet"].sample_size[1] * cfg["vae"].downscale
    return cfg, require_reprojectable(sensor_for(beams, **kw))


def masked_window(fraction, W, start=0.0):
    """[w0, w1) azimuth columns of the in-painting mask (ldm/dataset.py:348-362; w1 > W wraps past the seam)."""
    w0, end = int(start * W), start + fraction
    return (w0, int(end * W)) if end < 1.0 else (w0, W + int((end - 1.0) * W))


def _emit(result, json_path):
    text = json.dumps(result, sort_keys=True)
    print(text)
    if json_path:
        with open(json_path, "w") as f:
            f.write(text + "\n")


def _sum_over_ranks(values, device):
    """Element-wise fp64 sum of a list of floats over the ranks (identity on one process)."""
    t = torch.tensor(values, dtype=torch.float64, device=device)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().tolist()


def _load_bin(path, columns, device):
    return torch.from_numpy(np.fromfile(path, dtype=np.float32).reshape(-1, columns)).to(device)


def _chunks(seq, n):
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


def check_voxel_arg(a):
    """`--voxel`: refused before a file is read unless it is positive and finite (None: the flag was not given)."""
    if a.voxel is not None:
        from .metrics import _voxel_size
        _voxel_size(a.voxel)


def _occupancy_sums(result, target, voxel):
    """[sum iou, sum precision, sum recall, sum f1, sum a, sum b, sum c] over the pairs of one metrics.voxel_scores call
    (result clouds against target clouds): what a rank accumulates and _sum_over_ranks reduces."""
    from .metrics import VOXEL_SCORES, voxel_scores
    s = voxel_scores(result, target, voxel)
    return [float(s[k].sum()) for k in VOXEL_SCORES] + [float(v) for v in s["counts"].sum(0).tolist()]


def _occupancy_block(tot, n):
    """The "occupancy" object from the seven sums over all ranks and the number of pairs (the counts are integers below
    2^53: their fp64 sums are exact and order-free)."""
    from .metrics import VOXEL_SCORES
    out = {k: tot[i] / n for i, k in enumerate(VOXEL_SCORES)}
    out.update(voxels_result=int(tot[4]), voxels_target=int(tot[5]), voxels_both=int(tot[6]))
    return out


def _max_over_ranks(values, device):
    """Element-wise maximum of a list of floats over the ranks (identity on one process)."""
    t = torch.tensor(values, dtype=torch.float64, device=device)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.cpu().tolist()


def check_nn_args(a):
    """`--match` / `--dcd-alpha`: refused before a file is read unless positive and finite (None: the flag was not given)."""
    from .metrics import _alpha_value, _tau_values
    if a.match is not None:
        _tau_values(a.match)
    if a.dcd_alpha is not None:
        _alpha_value(a.dcd_alpha)


def _nn_wanted(a):
    return a.match is not None or a.dcd_alpha is not None


def _nn_len(a):
    """Length of _nn_sums' vector: with T thresholds [precision x T, recall x T, fscore x T, matched_result x T,
    matched_target x T, points_result, points_target, sum of Hausdorff], then [sum of dcd]."""
    return (5 * len(a.match) + 3 if a.match is not None else 0) + (1 if a.dcd_alpha is not None else 0)


def _nn_sums(result, target, a):
    """(sum of CD, the vector of _nn_len, the largest symmetric Hausdorff distance) over the pairs of ONE
    metrics.pair_scores call (result clouds against target clouds): what a rank accumulates; the first two are reduced by
    _sum_over_ranks, the last by _max_over_ranks."""
    from .metrics import pair_scores
    s = pair_scores(result, target, taus=a.match, alpha=a.dcd_alpha)
    sums, worst = [], 0.0
    if a.match is not None:
        m, h = s["match"], s["hausdorff"][:, 2]
        for k in ("precision", "recall", "fscore"):
            sums += m[k].sum(0).tolist()
        sums += [float(v) for v in m["counts"].sum(0).t().reshape(-1).tolist()]
        sums += [float(v) for v in m["points"].sum(0).tolist()] + [float(h.sum())]
        worst = float(h.max())
    if a.dcd_alpha is not None:
        sums.append(float(s["dcd"].sum()))
    return float(s["cd"].sum()), sums, worst


def _nn_blocks(tot, worst, n, a):
    """The "match" / "hausdorff" / "dcd" objects from _nn_sums' vector summed over all ranks, the maximum over all ranks and
    the number of pairs (the counts are integers below 2^53: their fp64 sums are exact and order-free)."""
    out = {}
    if a.match is not None:
        T = len(a.match)
        out["match"] = {"tau": list(a.match), **{k: [v / n for v in tot[i * T:(i + 1) * T]]
                                                 for i, k in enumerate(("precision", "recall", "fscore"))},
                        "matched_result": [int(v) for v in tot[3 * T:4 * T]], "matched_target": [int(v) for v in tot[4 * T:5 * T]],
                        "points_result": int(tot[5 * T]), "points_target": int(tot[5 * T + 1])}
        out["hausdorff"] = {"mean": tot[5 * T + 2] / n, "max": worst}
    if a.dcd_alpha is not None:
        out["dcd"] = {"alpha": a.dcd_alpha, "mean": tot[-1] / n}
    return out


def check_normals_arg(a):
    """`--normals`: refused before a file is read unless it is in 1..32 (None: the flag was not given)."""
    if a.normals is not None:
        from .metrics import _knn_k
        _knn_k(a.normals)


def _plane_sums(result, target, k):
    """[sum of cd_plane, sum of normal_consistency] over the pairs of one metrics.plane_scores call (result clouds against
    target clouds): what a rank accumulates and _sum_over_ranks reduces."""
    from .metrics import plane_scores
    s = plane_scores(result, target, k)
    return [float(s["cd_plane"].sum()), float(s["normal_consistency"].sum())]


def _plane_block(tot, n, k):
    return {"k": k, "cd_plane": tot[0] / n, "normal_consistency": tot[1] / n}


def _add(acc, part):
    return [s + t for s, t in zip(acc, part)]


# ---- commands ---------------------------------------------------------------------------------------------------------
def _load_vae(a):
    from .vae import AutoencoderKLHIP
    if a.sgm_ckpt:
        return AutoencoderKLHIP.from_sgm_checkpoint(a.sgm_ckpt, a.sgm_yaml), "sgm:" + os.path.basename(a.sgm_ckpt)
    if a.weights:
        sub = "vae" if os.path.isdir(os.path.join(a.weights, "vae")) else None
        return AutoencoderKLHIP.from_pretrained(a.weights, subfolder=sub), "diffusers:" + os.path.basename(a.weights)
    from .config import VAEConfig
    from .params import vae_param_shapes
    from .synth import synth_state_dict
    cfg = VAEConfig()
    vae = AutoencoderKLHIP(cfg)
    vae.load_state_dict(synth_state_dict(vae_param_shapes(cfg), seed=a.seed, prefix="vae."))
    return vae, "synthetic"


def cmd_vae(a, rank, world, dev):
    from .inference import sensor_for
    from .inference_conditional import load_batch
    from .metrics import chamfer_pairs, range_errors
    check_voxel_arg(a)
    check_nn_args(a)
    check_normals_arg(a)
    vae, origin = _load_vae(a)
    shape = (vae._cfg.in_channels, *vae._cfg.sample_size)
    files = sorted(glob.glob(os.path.join(a.input, "*.npy")))[:a.samples] if a.input else None
    total = len(files) if files is not None else a.samples
    if total == 0:
        raise ValueError(f"{a.input}: no .npy range images")
    to_range = sensor_for(shape[2])
    std, mean = range_affine(to_range)
    fill = float(to_range.range_fill_value[0])
    sums = [0.0, 0.0, 0.0, 0.0]                          # MAE, PSNR, CD, images
    occ = [0.0] * 7                                      # --voxel: _occupancy_sums
    nn, worst = [0.0] * _nn_len(a), 0.0                  # --match / --dcd-alpha: _nn_sums
    plane = [0.0, 0.0]                                   # --normals: _plane_sums
    n_batches = (total + a.batch_size - 1) // a.batch_size
    for b in range(rank, n_batches, world):              # batch b holds global samples [b * bs, (b + 1) * bs)
        lo, hi = b * a.batch_size, min(total, (b + 1) * a.batch_size)
        if files is not None:
            x = torch.from_numpy(np.stack([np.load(f).astype(np.float32) for f in files[lo:hi]]))
            if tuple(x.shape[1:]) != shape:
                raise ValueError(f"range images of shape {tuple(x.shape[1:])}, the VAE expects {shape}")
        else:
            x = load_batch(None, hi - lo, shape, a.seed + b)
        x = x.to(dev)
        rec = vae(x).sample                              # ldm/convert_vae.py:228
        # :236-247: channel 0 -> (x * std + mean) / range_fill_value[0], channel 1 as is; per-image mean over C x W x H
        sa, ss, count = range_errors(x, rec, scale=[std / fill, 1.0], shift=[mean / fill, 0.0])
        mse = (ss / count).cpu().tolist()
        sums[0] += float((sa / count).sum())
        sums[1] += sum(10.0 * math.log10(1.0 / m) if m > 0 else math.inf for m in mse)
        # :249-271: xyz of the returns closer than 70 m, input against reconstruction
        pin, cin = to_range.filter_points(to_range.to_pc_torch(x), 70.0)
        pout, cout = to_range.filter_points(to_range.to_pc_torch(rec), 70.0)
        cin, cout = cin.cpu().tolist(), cout.cpu().tolist()
        clouds_in = [pin[j, :cin[j], :3] for j in range(len(cin))]
        clouds_out = [pout[j, :cout[j], :3] for j in range(len(cout))]
        if _nn_wanted(a):                                # one search for the CD and the rest; result = reconstruction
            cd, part, w = _nn_sums(clouds_out, clouds_in, a)
            sums[2] += cd
            nn, worst = _add(nn, part), max(worst, w)
        else:
            xm, ym = chamfer_pairs(clouds_in, clouds_out)
            sums[2] += float((xm + ym).sum())
        sums[3] += hi - lo
        if a.voxel is not None:                          # the reconstruction is the result, the input the target
            occ = [s + t for s, t in zip(occ, _occupancy_sums(clouds_out, clouds_in, a.voxel))]
        if a.normals is not None:
            plane = _add(plane, _plane_sums(clouds_out, clouds_in, a.normals))
    mae, psnr, cd, n, *rest = _sum_over_ranks(sums + occ + plane + nn, dev)      # (occ, plane: zeros without their flags)
    occ, plane, nn = rest[:7], rest[7:9], rest[9:]
    result = {"task": "vae", "weights": origin, "samples": int(n), "mae": mae / n, "psnr": psnr / n, "cd": cd / n}
    if a.voxel is not None:
        result.update(voxel=a.voxel, occupancy=_occupancy_block(occ, n))
    if _nn_wanted(a):
        result.update(_nn_blocks(nn, _max_over_ranks([worst], dev)[0], n, a))
    if a.normals is not None:
        result["plane"] = _plane_block(plane, n, a.normals)
    return result


def _conditional_pairs(a, task):
    stem = "densification" if task == "upsample" else "inpainting"
    return pair_result_files(os.path.join(a.exp, f"{stem}_result"), os.path.join(a.exp, f"{stem}_target"))


def cmd_densification(a, rank, world, dev):
    from .metrics import beam_upsample, chamfer_pairs, range_errors
    check_voxel_arg(a)
    check_nn_args(a)
    check_normals_arg(a)
    cfg, sensor = task_sensor(a.cfg)
    if cfg["task"] != "upsample":
        raise ValueError(f"{a.cfg} is not an up-sampling config")
    std, mean = range_affine(sensor)
    rate, lim = cfg["rate"], cfg["range_limit"]
    pairs = _conditional_pairs(a, "upsample")
    methods = ("ours", "nearest", "bicubic")
    abs_sum = {m: 0.0 for m in methods}
    cd_sum = {m: 0.0 for m in methods}
    occ = {m: [0.0] * 7 for m in methods}                # --voxel: _occupancy_sums per method
    L = _nn_len(a)
    nn, worst = {m: [0.0] * L for m in methods}, {m: 0.0 for m in methods}      # --match / --dcd-alpha: _nn_sums per method
    plane = {m: [0.0, 0.0] for m in methods}              # --normals: _plane_sums per method
    W, H = sensor.width, sensor.H
    for chunk in _chunks(pairs[rank::world], 32):
        clouds = {m: [] for m in methods}
        targets = []
        for rpath, tpath in chunk:
            res, tgt = _load_bin(rpath, 4, dev), _load_bin(tpath, 4, dev)
            img_r, img_t = sensor.project(res)["jpg"][None], sensor.project(tgt)["jpg"][None]
            # baselines from every rate-th beam of the target starting at beam 0 (`target[::4]`, mae.py:61-81).  The
            # model's own condition takes beams rate//2, rate//2 + rate, ... (ldm/dataset.py:340-346): a quirk of the
            # reference, reproduced as it is
            low = img_t[..., ::rate].contiguous()
            imgs = {"ours": img_r, "nearest": beam_upsample(low, rate, "nearest"), "bicubic": beam_upsample(low, rate, "bicubic")}
            for m in methods:
                sa, _, _ = range_errors(imgs[m], img_t, scale=[std, 1.0], shift=[mean, 0.0], channels=[0])
                abs_sum[m] += float(sa.sum())
            targets.append(tgt[:, :3])
            clouds["ours"].append(res[:, :3])
            for m in ("nearest", "bicubic"):
                pts, cnt = sensor.filter_points(sensor.to_pc_torch(imgs[m]), lim)
                clouds[m].append(pts[0, :int(cnt[0]), :3])
        for m in methods:
            if _nn_wanted(a):                            # one search for the CD and the rest
                cd, part, w = _nn_sums(clouds[m], targets, a)
                cd_sum[m] += cd
                nn[m], worst[m] = _add(nn[m], part), max(worst[m], w)
            else:
                xm, ym = chamfer_pairs(clouds[m], targets)
                cd_sum[m] += float((xm + ym).sum())
            if a.voxel is not None:
                occ[m] = [s + t for s, t in zip(occ[m], _occupancy_sums(clouds[m], targets, a.voxel))]
            if a.normals is not None:
                plane[m] = _add(plane[m], _plane_sums(clouds[m], targets, a.normals))
    tot = _sum_over_ranks([abs_sum[m] for m in methods] + [cd_sum[m] for m in methods] +
                          [s for m in methods for s in occ[m]] + [s for m in methods for s in nn[m]] +
                          [s for m in methods for s in plane[m]], dev)
    n = len(pairs)
    result = {"task": "densification", "pairs": n, "rate": rate,
              "mae_m": {m: tot[i] / (n * W * H) for i, m in enumerate(methods)},
              "cd": {m: tot[3 + i] / n for i, m in enumerate(methods)}}
    if a.voxel is not None:
        result.update(voxel=a.voxel,
                      occupancy={m: _occupancy_block(tot[6 + 7 * i:13 + 7 * i], n) for i, m in enumerate(methods)})
    if _nn_wanted(a):                                    # one block per method, like "cd"
        worst = _max_over_ranks([worst[m] for m in methods], dev)
        blocks = [_nn_blocks(tot[27 + L * i:27 + L * (i + 1)], worst[i], n, a) for i in range(len(methods))]
        result.update({key: {m: blocks[i][key] for i, m in enumerate(methods)} for key in blocks[0]})
    if a.normals is not None:
        at = 27 + 3 * L
        result["plane"] = {m: _plane_block(tot[at + 2 * i:at + 2 * i + 2], n, a.normals) for i, m in enumerate(methods)}
    return result


def cmd_inpainting(a, rank, world, dev):
    from .metrics import chamfer_pairs, range_errors
    check_voxel_arg(a)
    check_nn_args(a)
    check_normals_arg(a)
    cfg, sensor = task_sensor(a.cfg)
    if cfg["task"] != "inpainting":
        raise ValueError(f"{a.cfg} is not an in-painting config")
    std, mean = range_affine(sensor)
    W, H = sensor.width, sensor.H
    w0, w1 = masked_window(cfg["fraction"], W)
    pairs = _conditional_pairs(a, "inpainting")
    abs_sum = cd_sum = 0.0
    occ = [0.0] * 7                                      # --voxel: _occupancy_sums
    nn, worst = [0.0] * _nn_len(a), 0.0                  # --match / --dcd-alpha: _nn_sums
    plane = [0.0, 0.0]                                   # --normals: _plane_sums
    for chunk in _chunks(pairs[rank::world], 32):
        res_c, tgt_c = [], []
        for rpath, tpath in chunk:
            res, tgt = _load_bin(rpath, 4, dev), _load_bin(tpath, 4, dev)
            sa, _, _ = range_errors(sensor.project(res)["jpg"][None], sensor.project(tgt)["jpg"][None], scale=[std, 1.0],
                                    shift=[mean, 0.0], channels=[0], window=(w0, w1))
            abs_sum += float(sa.sum())
            res_c.append(res[:, :3])
            tgt_c.append(tgt[:, :3])
        if _nn_wanted(a):                                # one search for the CD and the rest
            cd, part, w = _nn_sums(res_c, tgt_c, a)
            cd_sum += cd
            nn, worst = _add(nn, part), max(worst, w)
        else:
            xm, ym = chamfer_pairs(res_c, tgt_c)
            cd_sum += float((xm + ym).sum())
        if a.voxel is not None:
            occ = [s + t for s, t in zip(occ, _occupancy_sums(res_c, tgt_c, a.voxel))]
        if a.normals is not None:
            plane = _add(plane, _plane_sums(res_c, tgt_c, a.normals))
    abs_sum, cd_sum, *rest = _sum_over_ranks([abs_sum, cd_sum] + occ + plane + nn, dev)      # (occ, plane: zeros without their flags)
    occ, plane, nn = rest[:7], rest[7:9], rest[9:]
    n = len(pairs)
    result = {"task": "inpainting", "pairs": n, "window": [w0, w1],
              "mae_m": {"reference": abs_sum / (n * W * H),            # mae.py:111: divided by files x W x H (a quirk)
                        "per_masked_pixel": abs_sum / (n * (w1 - w0) * H)},
              "cd": cd_sum / n}
    if a.voxel is not None:
        result.update(voxel=a.voxel, occupancy=_occupancy_block(occ, n))
    if _nn_wanted(a):
        result.update(_nn_blocks(nn, _max_over_ranks([worst], dev)[0], n, a))
    if a.normals is not None:
        result["plane"] = _plane_block(plane, n, a.normals)
    return result


def cmd_chamfer(a, rank, world, dev):
    from .metrics import chamfer_pairs
    check_voxel_arg(a)
    check_nn_args(a)
    check_normals_arg(a)
    pairs = pair_by_name(a.a_dir, a.b_dir)
    cd = 0.0
    occ = [0.0] * 7                                      # --voxel: _occupancy_sums
    nn, worst = [0.0] * _nn_len(a), 0.0                  # --match / --dcd-alpha: _nn_sums
    plane = [0.0, 0.0]                                   # --normals: _plane_sums
    for chunk in _chunks(pairs[rank::world], 32):
        xs = [_load_bin(p, a.columns, dev)[:, :3] for p, _ in chunk]
        ys = [_load_bin(q, a.columns, dev)[:, :3] for _, q in chunk]
        if _nn_wanted(a):                                # one search for the CD and the rest
            c, part, w = _nn_sums(xs, ys, a)
            cd += c
            nn, worst = _add(nn, part), max(worst, w)
        else:
            xm, ym = chamfer_pairs(xs, ys)
            cd += float((xm + ym).sum())
        if a.voxel is not None:                          # A_DIR holds the results, B_DIR the targets
            occ = [s + t for s, t in zip(occ, _occupancy_sums(xs, ys, a.voxel))]
        if a.normals is not None:
            plane = _add(plane, _plane_sums(xs, ys, a.normals))
    cd, *rest = _sum_over_ranks([cd] + occ + plane + nn, dev)    # (occ, plane: zeros without their flags)
    occ, plane, nn = rest[:7], rest[7:9], rest[9:]
    result = {"task": "chamfer", "pairs": len(pairs), "cd": cd / len(pairs)}
    if a.voxel is not None:
        result.update(voxel=a.voxel, occupancy=_occupancy_block(occ, len(pairs)))
    if _nn_wanted(a):
        result.update(_nn_blocks(nn, _max_over_ranks([worst], dev)[0], len(pairs), a))
    if a.normals is not None:
        result["plane"] = _plane_block(plane, len(pairs), a.normals)
    return result


def _sum_matrix_over_ranks(m):
    """Element-wise sum of a device fp64 matrix over the ranks (identity on one process; gloo reduces host tensors)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return m
    if dist.get_backend() == "gloo":
        host = m.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM)
        return host.to(m.device)
    dist.all_reduce(m, op=dist.ReduceOp.SUM)
    return m


def _matrix_over_ranks(xs, ys, rank, world, matrix=None):
    """matrix(xs, ys) (ys None: xs against itself; default metrics.chamfer_matrix) with the rows shared out over the ranks:
    every rank writes its block of rows into a zero matrix and the sum over the ranks (adding zeros is exact) is the whole.
    A `matrix` passed in need not be symmetric in its arguments (an auction's matching of (a, b) is not that of (b, a)
    read backwards): its symmetric case takes entry [i][j], i < j, from (xs[i], xs[j]) as the one-process call does, and
    mirrors it."""
    from .metrics import chamfer_matrix
    mirror = matrix is not None and ys is None
    matrix = matrix or chamfer_matrix
    if world == 1:
        return matrix(xs, ys)
    cols = xs if ys is None else ys
    full = torch.zeros((len(xs), len(cols)), dtype=torch.float64, device=xs[0].device)
    lo, hi = D.shard_range(len(xs), rank, world)
    if hi > lo and mirror:
        full[lo:hi, lo:] = matrix(xs[lo:hi], xs[lo:])    # the columns left of the block lie below the diagonal
    elif hi > lo:
        full[lo:hi] = matrix(xs[lo:hi], cols)            # (a cloud against itself: every d^2 minimum is exactly 0)
    full = _sum_matrix_over_ranks(full)
    if mirror:
        upper = torch.triu(full, 1)
        full = upper + upper.t()
    return full


GENERATION_CHUNK = 256      # files read, cut and sub-sampled together (sampling="fps": one kernel launch per chunk)


def load_generation_clouds(files, columns, points, seed, max_depth, device, sampling="random"):
    """xyz of every file: the points closer than max_depth (None: all), then subsample(.., points, seed + file index,
    sampling), GENERATION_CHUNK files at a time through metrics.subsample_batch."""
    from .metrics import subsample_batch
    clouds = []
    for lo in range(0, len(files), GENERATION_CHUNK):
        chunk = []
        for path in files[lo:lo + GENERATION_CHUNK]:
            xyz = _load_bin(path, columns, device)[:, :3]
            if max_depth is not None:
                xyz = xyz[xyz.norm(dim=1) < max_depth]
            if xyz.shape[0] == 0:
                raise ValueError(f"{path}: no point left (max_depth={max_depth})")
            chunk.append(xyz)
        clouds.extend(subsample_batch(chunk, points, [seed + lo + i for i in range(len(chunk))], sampling))
    return clouds


def check_emd_args(a):
    """`generation --emd`: what can be refused before a file is read."""
    from .metrics import EMD_MAX_POINTS
    if a.points > EMD_MAX_POINTS:
        raise ValueError(f"--emd: --points {a.points} is above the {EMD_MAX_POINTS} points an EMD matching takes")
    if not (a.emd_eps > 0.0 and math.isfinite(a.emd_eps)):
        raise ValueError(f"--emd-eps must be positive and finite, got {a.emd_eps}")


def require_emd_sizes(files, clouds, points):
    """EMD is a one-to-one matching: every cloud must hold exactly `points` points; the first file that does not is named."""
    for path, cloud in zip(files, clouds):
        if int(cloud.shape[0]) != points:
            raise ValueError(f"{path}: {int(cloud.shape[0])} points are left, --emd needs --points {points} in every cloud "
                             f"(EMD is a one-to-one matching)")


def cmd_generation(a, rank, world, dev):
    from .metrics import evaluate_folders, set_metrics
    if a.emd:
        check_emd_args(a)
    gen_files = sorted(glob.glob(os.path.join(a.gen_dir, "*.bin")))[:a.limit]
    ref_files = sorted(glob.glob(os.path.join(a.ref_dir, "*.bin")))[:a.limit]
    if not gen_files or not ref_files:
        raise FileNotFoundError(f"no .bin files in {a.gen_dir if not gen_files else a.ref_dir}")
    gen = load_generation_clouds(gen_files, 4, a.points, a.seed, a.max_depth, dev, a.sampling)
    ref = load_generation_clouds(ref_files, a.columns, a.points, a.seed, a.max_depth, dev, a.sampling)
    if a.emd:
        require_emd_sizes(gen_files, gen, a.points)
        require_emd_sizes(ref_files, ref, a.points)
    result = {"task": "generation", "points": a.points}
    if a.sampling != "random":                           # (the default's object is what it was: no new key)
        result["sampling"] = a.sampling
    result.update(set_metrics(_matrix_over_ranks(gen, None, rank, world), _matrix_over_ranks(gen, ref, rank, world),
                              _matrix_over_ranks(ref, None, rank, world)))
    if a.emd:
        from .metrics import emd_matrix
        emd = lambda xs, ys: emd_matrix(xs, ys, eps=a.emd_eps)
        result.update(set_metrics(_matrix_over_ranks(gen, None, rank, world, emd), _matrix_over_ranks(gen, ref, rank, world, emd),
                                  _matrix_over_ranks(ref, None, rank, world, emd), name="emd"))
        result["emd_eps"] = a.emd_eps
    if rank == 0:                                        # the BEV histograms of the full clouds: cheap, one rank
        result.update(evaluate_folders(a.gen_dir, ref_files, nuscenes=a.columns == 5, limit=a.limit))
    return result


def check_frd_args(a):
    """`frd`: what can be refused before a file is read."""
    if a.limit < 2:
        raise ValueError(f"--limit must be at least 2 (a covariance needs 2 samples), got {a.limit}")
    if not 1 <= a.count <= a.total:
        raise ValueError(f"--count {a.count} values cannot be drawn from --total {a.total}")
    if getattr(a, "rangenet", None) and a.total != RANGENET_SHAPE[0] * RANGENET_SHAPE[1] * RANGENET_SHAPE[2]:
        raise ValueError(f"--rangenet draws from whole {RANGENET_SHAPE} feature maps: --total {a.total} does not apply")
    if getattr(a, "projection", "host") != "host" and not getattr(a, "rangenet", None):
        raise ValueError("--projection applies to point clouds: it needs --rangenet MODEL_DIR")


RANGENET_SHAPE = (32, 64, 1024)      # the activation of one scan: channels, beams, azimuth columns


def check_rangenet_args(a):
    """`rangenet`: what can be refused before a file is read."""
    if a.batch_size < 1:
        raise ValueError(f"--batch-size must be at least 1, got {a.batch_size}")
    dirs = {"--dump": a.dump, "--frd-dir": a.frd_dir, "--output-dir": a.output_dir}
    real = {k: os.path.realpath(v) for k, v in dirs.items()}
    labels_dir = getattr(a, "labels_dir", None)
    if labels_dir:
        real["--labels-dir"] = os.path.realpath(labels_dir)
    for k in ("--frd-dir", "--output-dir", "--labels-dir"):
        if k in real and real[k] == real["--dump"]:
            raise ValueError(f"{k} is the --dump folder: outputs are numbered files and must not land among the clouds")
    if getattr(a, "knn", False) and not labels_dir:
        raise ValueError("--knn cleans per-point labels: it needs --labels-dir")
    if labels_dir and getattr(a, "projection", "host") != "device":
        raise ValueError("--labels-dir needs --projection device (the host projection keeps no per-point pixels)")


def label_settings(model_dir, use_knn):
    """(knn params or None, uint32 lookup table or None) for `rangenet --labels-dir`: the post.KNN.params of the model's
    arch_cfg.yaml when --knn is given, and learning_map_inv of its data_cfg.yaml (class id -> SemanticKITTI label, the
    reference's to_original) when that file exists."""
    import yaml
    from .rangenet import NUM_CLASSES, knn_params
    knn = None
    if use_knn:
        with open(os.path.join(model_dir, "arch_cfg.yaml")) as f:
            knn = knn_params(yaml.safe_load(f))
    table = None
    path = os.path.join(model_dir, "data_cfg.yaml")
    if os.path.isfile(path):
        with open(path) as f:
            inv = yaml.safe_load(f)["learning_map_inv"]
        table = np.zeros(max(NUM_CLASSES, max(int(k) for k in inv) + 1), np.uint32)
        for k, v in inv.items():
            table[int(k)] = int(v)
    return knn, table


def check_segmentation_args(a):
    """`segmentation`: what can be refused before a file is read."""
    if not 1 <= a.classes <= 256:
        raise ValueError(f"--classes must be in [1, 256], got {a.classes}")


def _cloud_files(folder, limit=None):
    files = sorted(glob.glob(os.path.join(folder, "*.bin")))[:limit]
    if not files:
        raise FileNotFoundError(f"no .bin point clouds in {folder}")
    return files


def _project_files_device(files, dev):
    """rangenet.ProjectedScans of the x y z remission clouds: read, packed on the host, one upload, one projection call."""
    from .rangenet import project_scans
    _, H, W = RANGENET_SHAPE
    clouds = [np.fromfile(path, dtype=np.float32).reshape(-1, 4) for path in files]
    return project_scans(np.concatenate(clouds, 0), [c.shape[0] for c in clouds], H=H, W=W, device=dev)


def _project_files(files, dev, projection="host"):
    """(len(files), 5, 64, 1024) on the device: rangenet.project_scan of every x y z remission cloud (projection "device":
    rangenet.project_scans of all of them at once)."""
    from .rangenet import project_scan
    if projection == "device":
        return _project_files_device(files, dev).proj
    _, H, W = RANGENET_SHAPE
    out = np.empty((len(files), 5, H, W), np.float32)
    for i, path in enumerate(files):
        scan = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
        out[i], _ = project_scan(scan[:, :3], scan[:, 3], H=H, W=W)
    return torch.from_numpy(out).to(dev)


def rangenet_activations(net, folder, idx, limit, rank, world, dev, batch_size=4, projection="host"):
    """(files, len(idx)) fp32: the drawn values of every cloud's activation, the clouds shared out over the ranks (rank r takes
    i = r, r + world, ...; the rows of the others are zero until the sum over the ranks, which adds zeros: exact)."""
    files = _cloud_files(folder, limit)
    rows = torch.zeros((len(files), len(idx)), dtype=torch.float32, device=dev)
    mine = list(range(rank, len(files), world))
    for chunk in _chunks(mine, batch_size):
        _, gathered = net.infer(_project_files([files[i] for i in chunk], dev, projection), gather=idx)
        rows[torch.as_tensor(chunk, device=dev)] = gathered
    return _sum_matrix_over_ranks(rows)


def cmd_frd(a, rank, world, dev):
    from .metrics import frd_indices, frechet_distance, load_activations
    check_frd_args(a)
    if a.rangenet:                                       # the forwards are shared out; rank 0 then goes on alone
        from .rangenet import RangeNet
        net = RangeNet.from_pretrained(a.rangenet, device=dev)
        idx = frd_indices(a.total, a.count)
        x = rangenet_activations(net, a.folder1, idx, a.limit, rank, world, dev, projection=a.projection)
        y = rangenet_activations(net, a.folder2, idx, a.limit, rank, world, dev, projection=a.projection)
        if rank != 0:
            return None
    else:
        if rank != 0:                                    # one small matrix: nothing to shard
            return None
        idx = frd_indices(a.total, a.count)
        x = load_activations(a.folder1, idx, a.limit, a.total, dev)
        y = load_activations(a.folder2, idx, a.limit, a.total, dev)
    terms = frechet_distance(x, y, return_terms=True)
    result = {"task": "frd", **terms, "n1": int(x.shape[0]), "n2": int(y.shape[0]), "dims": int(x.shape[1])}
    if a.projection != "host":                           # (the default's object is what it was: no new key)
        result["projection"] = a.projection
    return result


def check_features_args(a):
    """`features`: what can be refused before a file is read."""
    from .metrics import FEATURE_K_CAP
    if not 1 <= a.k <= FEATURE_K_CAP:
        raise ValueError(f"--k must be in [1, {FEATURE_K_CAP}], got {a.k}")
    if a.limit is not None and a.limit < a.k + 1:
        raise ValueError(f"--limit must be at least --k + 1 = {a.k + 1} (a row's neighbourhood counts the row itself), got {a.limit}")
    if a.subset_size is not None and a.subset_size < 2:
        raise ValueError(f"--subset-size must be at least 2, got {a.subset_size}")
    if a.subsets < 1:
        raise ValueError(f"--subsets must be at least 1, got {a.subsets}")
    if not 1 <= a.count <= a.total:
        raise ValueError(f"--count {a.count} values cannot be drawn from --total {a.total}")
    if a.rangenet and a.total != RANGENET_SHAPE[0] * RANGENET_SHAPE[1] * RANGENET_SHAPE[2]:
        raise ValueError(f"--rangenet draws from whole {RANGENET_SHAPE} feature maps: --total {a.total} does not apply")
    if a.projection != "host" and not a.rangenet:
        raise ValueError("--projection applies to point clouds: it needs --rangenet MODEL_DIR")


def cmd_features(a, rank, world, dev):
    from .metrics import frd_indices, kernel_distance, load_activations, prdc
    check_features_args(a)
    idx = frd_indices(a.total, a.count)
    if a.rangenet:                                       # the forwards are shared out; rank 0 then goes on alone
        from .rangenet import RangeNet
        net = RangeNet.from_pretrained(a.rangenet, device=dev)
        gen = rangenet_activations(net, a.gen_dir, idx, a.limit, rank, world, dev, projection=a.projection)
        ref = rangenet_activations(net, a.ref_dir, idx, a.limit, rank, world, dev, projection=a.projection)
        if rank != 0:
            return None
    else:
        if rank != 0:                                    # two small matrices: nothing to shard
            return None
        gen = load_activations(a.gen_dir, idx, a.limit, a.total, dev)
        ref = load_activations(a.ref_dir, idx, a.limit, a.total, dev)
    result = {"task": "features", "k": a.k, "n_gen": int(gen.shape[0]), "n_ref": int(ref.shape[0]), "dims": int(gen.shape[1])}
    if a.subset_size is None:
        result["krd"] = kernel_distance(gen, ref)
    else:
        result.update(kernel_distance(gen, ref, subset_size=a.subset_size, subsets=a.subsets, seed=a.seed),
                      subsets=a.subsets, subset_size=a.subset_size)
    result.update(prdc(ref, gen, k=a.k))
    if a.projection != "host":
        result["projection"] = a.projection
    return result


def cmd_rangenet(a, rank, world, dev):
    from .rangenet import RangeNet
    check_rangenet_args(a)
    files = _cloud_files(a.dump)
    net = RangeNet.from_pretrained(a.model, device=dev)
    knn, to_original = None, None
    if a.labels_dir:
        knn, to_original = label_settings(a.model, a.knn)
    for d in (a.frd_dir, a.output_dir, a.labels_dir):
        if d:
            os.makedirs(d, exist_ok=True)
    for chunk in _chunks(list(range(rank, len(files), world)), a.batch_size):
        names = [files[i] for i in chunk]
        scans = _project_files_device(names, dev) if a.projection == "device" else None
        argmax, features = net.infer(scans.proj if scans is not None else _project_files(names, dev))
        if a.labels_dir:
            from .rangenet import unproject
            labels = scans.split(unproject(scans, argmax, knn).cpu())
        features, argmax = features.cpu().numpy(), argmax.cpu().to(torch.int64)
        for k, i in enumerate(chunk):
            np.save(os.path.join(a.frd_dir, f"{i}.npy"), features[k:k + 1])      # (1, 32, 64, 1024), as Decoder.forward saves it
            torch.save(argmax[k].clone(), os.path.join(a.output_dir, f"{i}.pth"))
            if a.labels_dir:
                lab = labels[k].numpy().astype(np.uint32)
                (to_original[lab] if to_original is not None else lab).astype(np.uint32).tofile(os.path.join(a.labels_dir, f"{i}.label"))
    result = {"task": "rangenet", "files": len(files), "layers": net.layers}
    if a.projection != "host":                           # (the default's object is what it was: no new keys)
        result["projection"] = a.projection
    if a.labels_dir:
        result["labels"] = "knn" if a.knn else "plain"
    return result


def cmd_segmentation(a, rank, world, dev):
    from .rangenet import confusion_matrix, scores_from_confusion
    check_segmentation_args(a)
    res = {os.path.basename(p) for p in glob.glob(os.path.join(a.result_dir, "*.pth"))}
    tgt = {os.path.basename(p) for p in glob.glob(os.path.join(a.target_dir, "*.pth"))}
    if not tgt:
        raise FileNotFoundError(f"no .pth label tensors in {a.target_dir}")
    if res != tgt:
        raise FileNotFoundError(f"{a.result_dir} and {a.target_dir} do not hold the same .pth names "
                                f"(for instance {sorted(res ^ tgt)[0]})")
    names = sorted(tgt)
    cm = torch.zeros((a.classes, a.classes), dtype=torch.int64, device=dev)
    for name in names[rank::world]:
        pred = torch.load(os.path.join(a.result_dir, name), map_location="cpu", weights_only=True)
        target = torch.load(os.path.join(a.target_dir, name), map_location="cpu", weights_only=True)
        cm += confusion_matrix(pred.to(dev), target.to(dev), a.classes)
    # integer counts below 2^53: their fp64 sum over the ranks is exact and order-free
    cm = torch.tensor(_sum_over_ranks(cm.reshape(-1).tolist(), dev), dtype=torch.float64).to(torch.int64).reshape(a.classes, a.classes)
    return {"task": "segmentation", **scores_from_confusion(cm), "n": len(names)}


COMMANDS = {"features": cmd_features, "rangenet": cmd_rangenet, "segmentation": cmd_segmentation, "frd": cmd_frd, "generation": cmd_generation, "vae": cmd_vae, "densification": cmd_densification, "inpainting": cmd_inpainting, "chamfer": cmd_chamfer}


def main(argv=None):
    a = build_parser().parse_args(argv)
    rank, world, local = D.init_from_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    result = COMMANDS[a.cmd](a, rank, world, dev)
    if rank == 0:
        _emit(result, a.json)
    D.barrier()
    return result


if __name__ == "__main__":
    main()
