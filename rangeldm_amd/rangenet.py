"""RangeNet++ inference on the MI355X: the DarkNet21 / DarkNet53 segmentation network whose last decoder feature map is the
FRD activation (`N.npy`) and whose per-pixel argmax is the segmentation (`N.pth`) that `metric.py --iou / --accuracy` compare
(metrics/rangenetpp/lidar_bonnetal_master/train: backbones/darknet.py, tasks/semantic/decoders/darknet.py,
tasks/semantic/modules/segmentator.py:47-50, 149-153; metrics/metrics/iou.py).

    net = RangeNet.from_pretrained("darknet53-1024")          # arch_cfg.yaml + backbone / segmentation_decoder / segmentation_head
    proj, mask = project_scan(points, remission)              # host: LaserScan.do_range_projection + the parser's normalisation
    argmax, features = net.infer(torch.from_numpy(proj)[None].cuda())
    scans = project_scans([cloud0, cloud1])                   # device: a ragged batch of (N, 4) clouds -> scans.proj (B, 5, H, W)
    labels = net.segment([cloud0, cloud1], knn=knn_params(arch))     # per-point uint8 labels, one array per cloud

The forward runs in librangeldm_hip (csrc/rangenet.hip): one launch per layer, bf16 activations, fp32 accumulation.  A layer is

    acc = sum_taps W . X                 zeros outside the image on both axes
    v   = acc * scale[c] + shift[c]      BatchNorm (eval) folded: scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale
                                         (+ bias * scale); kept in fp32, NOT folded into the bf16 weights
    v   = v >= 0 ? v : 0.1f * v          LeakyReLU(0.1)
    v   = v + add0 + add1                BasicBlock residual, then the decoder's skip
    out = bf16(v)

`layer_host` and `forward_host` restate that in plain torch on the CPU (the house pattern of metrics.frechet_distance_host): fp32
throughout, or with bf16=True rounded to bf16 at exactly the points where the kernel rounds.

Around the forward (csrc/rangenet_post.hip): `project_scans` projects a ragged batch of scans on the device (`project_scan` is
the host's, one scan at a time, and stays what it was), `unproject` takes the argmax back to per-point labels, plainly
(`argmax[py, px]`) or through the reference's KNN vote (postproc/KNN.py), and `RangeNet.segment` chains the three.
`scatter_host` and `knn_labels_host` restate the two device rules in numpy.

Not built, refused with NotImplementedError: backbones / decoders other than `darknet`, CRF, output strides other than 32, inputs
other than the five channels (range, x, y, z, remission).  An arch_cfg with `post.KNN.use: True` is refused as well: KNN is
asked for explicitly (`segment(knn=...)`, `evaluate rangenet --knn`), with the params the arch_cfg carries.
"""
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import synth

MODEL_BLOCKS = {21: (1, 1, 2, 2, 1), 53: (1, 2, 8, 8, 4)}          # backbones/darknet.py model_blocks
NUM_CLASSES = 20
FEATURE_CHANNELS = 32
BN_EPS = 1e-5
# darknet53-1024/arch_cfg.yaml dataset.sensor: range, x, y, z, remission
IMG_MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)
IMG_STDS = (12.32, 11.47, 6.91, 0.86, 0.16)
KIND_1X1, KIND_3X3, KIND_3X3_S2, KIND_UPCONV = (_lib.RLDM_RN_CONV1X1, _lib.RLDM_RN_CONV3X3, _lib.RLDM_RN_CONV3X3_S2,
                                                _lib.RLDM_RN_UPCONV)


def pitch(c):
    """Channels of a device activation holding c logical channels (RLDM_RN_PITCH)."""
    return (c + 15) & ~15


# ---- the architecture ----------------------------------------------------------------------------------------------------
def synthetic_arch(layers=53):
    """The parts of darknet53-1024/arch_cfg.yaml the network depends on."""
    return {"backbone": {"name": "darknet", "input_depth": {"range": True, "xyz": True, "remission": True}, "dropout": 0.05,
                         "bn_d": 0.01, "OS": 32, "train": True, "extra": {"layers": int(layers)}},
            "decoder": {"name": "darknet", "dropout": 0.05, "bn_d": 0.01, "train": True, "extra": False},
            "head": {"name": "segmentation", "train": True, "dropout": 0.05},
            "post": {"CRF": {"use": False, "train": True, "params": False},
                     "KNN": {"use": False, "params": {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}}}}


def check_arch(arch):
    """The number of DarkNet layers (21 or 53) of an arch_cfg dict; NotImplementedError for what is not built."""
    bb, dec, post = arch["backbone"], arch["decoder"], arch.get("post", {})
    if bb["name"] != "darknet":
        raise NotImplementedError(f"backbone {bb['name']!r}: only the darknet backbone is built")
    if dec["name"] != "darknet":
        raise NotImplementedError(f"decoder {dec['name']!r}: only the darknet decoder is built")
    if post.get("CRF", {}).get("use"):
        raise NotImplementedError("CRF post-processing is not built")
    if post.get("KNN", {}).get("use"):
        raise NotImplementedError("KNN post-processing is not built")
    if int(bb["OS"]) != 32:
        raise NotImplementedError(f"output stride {bb['OS']}: only OS 32 (five azimuth halvings) is built")
    depth = bb.get("input_depth", {})
    if not (depth.get("range") and depth.get("xyz") and depth.get("remission")):
        raise NotImplementedError("only the five-channel input (range, xyz, remission) is built")
    layers = int(bb["extra"]["layers"])
    if layers not in MODEL_BLOCKS:
        raise NotImplementedError(f"DarkNet{layers}: only DarkNet21 and DarkNet53 are built")
    return layers


def layer_specs(layers):
    """The layers in walk order (the order of rldm_rangenet_layer_info): dicts of kind, cin, cout, leaky, and where the
    weights live: `part` (backbone / decoder / head), `conv` and `bn` key prefixes (bn None: no BatchNorm), `bias`."""
    specs = []

    def push(kind, cin, cout, part, conv, bn, bias=False, leaky=True):
        specs.append({"kind": kind, "cin": cin, "cout": cout, "leaky": leaky, "part": part, "conv": conv, "bn": bn, "bias": bias})

    push(KIND_3X3, 5, 32, "backbone", "conv1", "bn1")
    c = 32
    for l, n in enumerate(MODEL_BLOCKS[layers], 1):
        push(KIND_3X3_S2, c, 2 * c, "backbone", f"enc{l}.conv", f"enc{l}.bn")
        for k in range(n):
            push(KIND_1X1, 2 * c, c, "backbone", f"enc{l}.residual_{k}.conv1", f"enc{l}.residual_{k}.bn1")
            push(KIND_3X3, c, 2 * c, "backbone", f"enc{l}.residual_{k}.conv2", f"enc{l}.residual_{k}.bn2")
        c *= 2
    for l in range(5, 0, -1):
        push(KIND_UPCONV, c, c // 2, "decoder", f"dec{l}.upconv", f"dec{l}.bn", bias=True)
        push(KIND_1X1, c // 2, c, "decoder", f"dec{l}.residual.conv1", f"dec{l}.residual.bn1")
        push(KIND_3X3, c, c // 2, "decoder", f"dec{l}.residual.conv2", f"dec{l}.residual.bn2")
        c //= 2
    push(KIND_3X3, 32, NUM_CLASSES, "head", "1", None, bias=True, leaky=False)
    return specs


def bn_names(layers):
    """`part.prefix` of every BatchNorm in walk order."""
    return [f"{s['part']}.{s['bn']}" for s in layer_specs(layers) if s["bn"]]


def bn_stats_from_arrays(layers, mean, var):
    """{`part.prefix`: (running_mean, running_var)} from the two arrays that hold every BatchNorm's statistics one after another
    in walk order (how tests/golden/rangenet.npz stores a calibrated set, as fp16: the values ARE the fp16 ones)."""
    mean, var = np.asarray(mean).astype(np.float32), np.asarray(var).astype(np.float32)
    out, at = {}, 0
    for s in layer_specs(layers):
        if s["bn"]:
            out[f"{s['part']}.{s['bn']}"] = (mean[at:at + s["cout"]], var[at:at + s["cout"]])
            at += s["cout"]
    if at != mean.shape[0] or at != var.shape[0]:
        raise ValueError(f"DarkNet{layers} holds {at} BatchNorm channels, got {mean.shape[0]} means and {var.shape[0]} variances")
    return out


def synthetic_state(arch, seed=synth.DEFAULT_SEED, bn_stats=None, head_bias_std=0.02):
    """(backbone_sd, decoder_sd, head_sd) of fp32 torch tensors in the reference's naming, identical on every machine: conv weights
    are synth.normal streams keyed by their names and He-scaled for LeakyReLU(0.1) (std = sqrt(2 / (1.01 fan_in))); biases
    0.02 * normal; BatchNorm weight 1 + 0.1 * uniform, bias 0.1 * uniform.  bn_stats: {`part.prefix`: (running_mean,
    running_var)} (tests/golden/rangenet.npz holds a calibrated set); missing entries are mean 0, variance 1.  head_bias_std: the spread of the head's
    class biases (class priors).  It is what sets how wide the top-2 logit margins are against the network's rounding noise: scaling
    the head's WEIGHTS scales margin and noise alike."""
    layers = check_arch(arch)
    sds = {"backbone": {}, "decoder": {}, "head": {}}
    for s in layer_specs(layers):
        sd, name = sds[s["part"]], f"{s['part']}.{s['conv']}"
        if s["kind"] == KIND_UPCONV:
            shape, fan_in = (s["cin"], s["cout"], 1, 4), 2 * s["cin"]         # two taps reach every output column
        else:
            k = 1 if s["kind"] == KIND_1X1 else 3
            shape, fan_in = (s["cout"], s["cin"], k, k), s["cin"] * k * k
        w = synth.normal(seed, name + ".weight", shape) * np.float32(np.sqrt(2.0 / (1.01 * fan_in)))
        sd[s["conv"] + ".weight"] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        if s["bias"]:
            std = head_bias_std if s["part"] == "head" else 0.02
            sd[s["conv"] + ".bias"] = torch.from_numpy(np.float32(std) * synth.normal(seed, name + ".bias", (s["cout"],)))
        if s["bn"]:
            key = f"{s['part']}.{s['bn']}"
            mean, var = (bn_stats or {}).get(key, (np.zeros(s["cout"], np.float32), np.ones(s["cout"], np.float32)))
            sd[s["bn"] + ".weight"] = torch.from_numpy(1.0 + np.float32(0.1) * synth.uniform(seed, key + ".weight", (s["cout"],)))
            sd[s["bn"] + ".bias"] = torch.from_numpy(np.float32(0.1) * synth.uniform(seed, key + ".bias", (s["cout"],)))
            sd[s["bn"] + ".running_mean"] = torch.from_numpy(np.asarray(mean, dtype=np.float32).copy())
            sd[s["bn"] + ".running_var"] = torch.from_numpy(np.asarray(var, dtype=np.float32).copy())
            sd[s["bn"] + ".num_batches_tracked"] = torch.tensor(1, dtype=torch.int64)
    return sds["backbone"], sds["decoder"], sds["head"]


def fold_state(arch, backbone_sd, decoder_sd, head_sd):
    """The network as the kernel sees it: {"layers": 21 | 53, "specs": [...]}, one spec per layer in walk order with `w` (fp32, the
    reference's layout: conv (Cout, Cin, k, k), up-conv (Cin, Cout, 1, 4)), `scale`, `shift` (fp32 (Cout,), BatchNorm and bias
    folded in fp32), `bias` (the conv's own, or None) and kind / cin / cout / leaky."""
    layers = check_arch(arch)
    sds = {"backbone": backbone_sd, "decoder": decoder_sd, "head": head_sd}
    out = []
    for s in layer_specs(layers):
        sd = sds[s["part"]]

        def get(key):
            if key not in sd:
                raise KeyError(f"{s['part']} state dict has no {key!r}")
            return torch.as_tensor(sd[key]).detach().to("cpu", torch.float32)

        w = get(s["conv"] + ".weight").contiguous()
        want = (s["cin"], s["cout"], 1, 4) if s["kind"] == KIND_UPCONV else \
            (s["cout"], s["cin"]) + ((1, 1) if s["kind"] == KIND_1X1 else (3, 3))
        if tuple(w.shape) != want:
            raise ValueError(f"{s['part']}.{s['conv']}.weight has shape {tuple(w.shape)}, expected {want}")
        if s["bn"]:
            scale = get(s["bn"] + ".weight") / torch.sqrt(get(s["bn"] + ".running_var") + BN_EPS)
            shift = get(s["bn"] + ".bias") - get(s["bn"] + ".running_mean") * scale
        else:
            scale, shift = torch.ones(s["cout"]), torch.zeros(s["cout"])
        bias = get(s["conv"] + ".bias") if s["bias"] else None
        if bias is not None:
            shift = shift + bias * scale
        out.append({"kind": s["kind"], "cin": s["cin"], "cout": s["cout"], "leaky": s["leaky"], "w": w, "bias": bias,
                    "scale": scale.contiguous(), "shift": shift.contiguous()})
    return {"layers": layers, "specs": out}


# ---- the host restatement ------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def upconv_by_parity(x, w):
    """ConvTranspose2d(kernel [1,4], stride [1,2], padding [0,1]) without bias as the kernel runs it: two 2-tap convs by
    output-column parity, zeros outside the image.  x (B, Cin, H, W), w (Cin, Cout, 1, 4) -> (B, Cout, H, 2 W):
    out[2j] = W[..,1] x[j] + W[..,3] x[j-1], out[2j+1] = W[..,2] x[j] + W[..,0] x[j+1]."""
    B, _, H, W = x.shape
    tap = lambda k, xs: torch.einsum("io,bihw->bohw", w[:, :, 0, k], xs)
    left = F.pad(x, (1, 0))[..., :W]                     # x[j-1]
    right = F.pad(x, (0, 1))[..., 1:]                    # x[j+1]
    out = x.new_empty((B, w.shape[1], H, 2 * W))
    out[..., 0::2] = tap(1, x) + tap(3, left)
    out[..., 1::2] = tap(2, x) + tap(0, right)
    return out


def layer_host(kind, x, w, scale, shift, leaky=True, add0=None, add1=None, bf16=False):
    """One layer on the CPU in fp32 torch, step by step as the kernel computes it: x (B, Cin, H, W), w in the reference's
    layout, scale / shift (Cout,), add0 / add1 of the output's shape -> (out, v): v the fp32 value before the final rounding
    (the kernel's fp32 store), out = v rounded to bf16 (as fp32) when bf16 else v.  With bf16=True x, w and the addends are
    rounded to bf16 first: the kernel's operands."""
    x = x.to(torch.float32)
    w, scale, shift = (t.to(x.device, torch.float32) for t in (w, scale, shift))
    if bf16:
        x, w = _bf16(x), _bf16(w)
    if kind == KIND_UPCONV:
        acc = F.conv_transpose2d(x, w, stride=(1, 2), padding=(0, 1))
    elif kind == KIND_1X1:
        acc = F.conv2d(x, w)
    else:
        acc = F.conv2d(x, w, stride=(1, 2 if kind == KIND_3X3_S2 else 1), padding=1)
    v = acc * scale.view(1, -1, 1, 1)
    v = v + shift.view(1, -1, 1, 1)
    if leaky:
        v = torch.where(v >= 0, v, v * torch.tensor(0.1, dtype=torch.float32, device=x.device))
    for add in (add0, add1):
        if add is not None:
            add = add.to(x.device, torch.float32)
            v = v + (_bf16(add) if bf16 else add)
    return (_bf16(v) if bf16 else v), v


def state_to(state, device):
    """The folded state with its tensors on `device` (forward_host then runs there without copying per layer)."""
    move = lambda s: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in s.items()}
    return {"layers": state["layers"], "specs": [move(s) for s in state["specs"]]}


def network_flops(state, H, W):
    """Multiply-adds x 2 of one scan's forward (the taps that reach an output: two for the transposed conv)."""
    total, w = 0, W
    for s in state["specs"]:
        taps = {KIND_1X1: 1, KIND_3X3: 9, KIND_3X3_S2: 9, KIND_UPCONV: 2}[s["kind"]]
        w = w // 2 if s["kind"] == KIND_3X3_S2 else 2 * w if s["kind"] == KIND_UPCONV else w
        total += 2 * s["cin"] * s["cout"] * taps * H * w
    return total


def forward_host(state, proj, bf16=False, return_rms=False, calibrate=None, device="cpu"):
    """The whole forward in plain torch (on the CPU unless `device` says otherwise): proj (B, 5, H, W) fp32 -> (features (B, 32, H, W) fp32, logits (B, 20, H, W) fp32);
    with bf16=True every conv's operands and every stored activation are rounded to bf16 where the kernel rounds (the features
    and the logits are its fp32 stores, before a rounding).  return_rms: also the RMS of every layer's output, in walk order.
    calibrate: a list that receives (mean, biased variance) of every BatchNorm layer's conv output; the layer then normalises with
    those instead of its folded statistics (tools/make_rangenet_golden.py: the calibration pass)."""
    specs, layers = state["specs"], state["layers"]
    it = iter(specs)
    rms = []

    def run(x, add0=None, add1=None, has_bn=True):
        s = next(it)
        scale, shift = s["scale"], s["shift"]
        if calibrate is not None and has_bn:
            _, acc = layer_host(s["kind"], x, s["w"], torch.ones_like(scale), torch.zeros_like(shift), leaky=False, bf16=bf16)
            mean, var = acc.mean(dim=(0, 2, 3)), acc.var(dim=(0, 2, 3), unbiased=False)
            # the state was folded with mean 0, variance 1: scale = gamma / sqrt(1 + eps), shift = beta + bias * scale.  Re-fold
            # with the statistics of the BatchNorm's input (the conv output plus its bias)
            bias = s["bias"] if s["bias"] is not None else torch.zeros_like(shift)
            beta = shift - bias * scale
            gamma = scale * float(np.sqrt(1.0 + BN_EPS))
            calibrate.append((mean + bias, var.clone()))
            scale = gamma / torch.sqrt(var + BN_EPS)
            shift = beta - mean * scale
        out, v = layer_host(s["kind"], x, s["w"], scale, shift, s["leaky"], add0, add1, bf16)
        rms.append(float(v.pow(2).mean().sqrt()))
        return out, v

    x = proj.to(device, torch.float32)
    x, _ = run(x)
    skips = []
    for n in MODEL_BLOCKS[layers]:
        skips.append(x)                                  # skips[os]: the input of the down-sampler
        x, _ = run(x)
        for _ in range(n):
            y, _ = run(x)
            x, _ = run(y, add0=x)
    v = None
    for l in range(4, -1, -1):
        d, _ = run(x)
        y, _ = run(d)
        x, v = run(y, add0=d, add1=skips[l])
    _, logits = run(x, has_bn=False)
    return (v, logits, rms) if return_rms else (v, logits)


# ---- the projection (host) -----------------------------------------------------------------------------------------------
def project_scan(points, remission=None, H=64, W=1024, fov_up=3.0, fov_down=-25.0, means=IMG_MEANS, stds=IMG_STDS):
    """LaserScan.do_range_projection (modules/kittiparser.py:111-171) and the parser's normalisation (:391-395) in numpy:
    points (N, 3) float32, remission (N,) float32 or None -> (proj (5, H, W) float32: range, x, y, z, remission, normalised
    and masked; mask (H, W) float32).  Points are written in order of decreasing depth, so the nearest wins a pixel; the mask is
    the reference's `proj_idx > 0`, which also drops the pixel that point 0 wins.  Depth ties are written in the order of the
    reference's `argsort` (numpy's default, unstable: undefined for equal depths)."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N, 3), got {points.shape}")
    n = points.shape[0]
    remission = np.zeros(n, np.float32) if remission is None else np.ascontiguousarray(remission, dtype=np.float32).reshape(-1)
    if remission.shape[0] != n:
        raise ValueError(f"{remission.shape[0]} remissions for {n} points")
    fov_up_r = fov_up / 180.0 * np.pi
    fov_down_r = fov_down / 180.0 * np.pi
    fov = abs(fov_down_r) + abs(fov_up_r)
    depth = np.linalg.norm(points, 2, axis=1)
    scan_x, scan_y, scan_z = points[:, 0], points[:, 1], points[:, 2]
    yaw = -np.arctan2(scan_y, scan_x)
    pitch_ = np.arcsin(scan_z / depth)
    proj_x = 0.5 * (yaw / np.pi + 1.0)
    proj_y = 1.0 - (pitch_ + abs(fov_down_r)) / fov
    proj_x *= W
    proj_y *= H
    proj_x = np.maximum(0, np.minimum(W - 1, np.floor(proj_x))).astype(np.int32)
    proj_y = np.maximum(0, np.minimum(H - 1, np.floor(proj_y))).astype(np.int32)
    order = np.argsort(depth)[::-1]
    proj_range = np.full((H, W), -1, dtype=np.float32)
    proj_xyz = np.full((H, W, 3), -1, dtype=np.float32)
    proj_rem = np.full((H, W), -1, dtype=np.float32)
    proj_idx = np.full((H, W), -1, dtype=np.int32)
    py, px = proj_y[order], proj_x[order]
    proj_range[py, px] = depth[order]
    proj_xyz[py, px] = points[order]
    proj_rem[py, px] = remission[order]
    proj_idx[py, px] = np.arange(n)[order]
    mask = (proj_idx > 0).astype(np.float32)
    proj = np.concatenate([proj_range[None], proj_xyz.transpose(2, 0, 1), proj_rem[None]], 0)
    proj = (proj - np.asarray(means, np.float32)[:, None, None]) / np.asarray(stds, np.float32)[:, None, None]
    return (proj * mask).astype(np.float32), mask


# ---- the projection (device) and its restatement -------------------------------------------------------------------------
class ProjectedScans:
    """What project_scans returns, all on the device: proj (B, 5, H, W) fp32, mask (B, H, W) fp32, proj_range (B, H, W) fp32
    (-1 where empty), proj_idx (B, H, W) int32 (the winner's index in its cloud, -1 where empty), px / py (sum N,) int32
    (-1: the point was dropped), unproj_range (sum N,) fp32, offsets (B + 1,) int32; `lengths` is the host's list of N_i."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def split(self, per_point):
        """A per-point device tensor (sum N, ...) as a list of per-cloud views."""
        return list(torch.split(per_point, self.lengths))


def pack_clouds(clouds, lengths=None, device="cuda"):
    """(points (sum N, 4) fp32 on the device, lengths): from a list of (N_i, 4) or (N_i, 3) arrays / tensors (three columns:
    remission 0), or from a packed (sum N, 3 | 4) array / tensor and its lengths.  Host arrays are joined on the host and go
    up in one copy."""
    def four(a):
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError(f"a cloud must be (N, 3) or (N, 4), got {tuple(a.shape)}")
        if a.shape[1] == 4:
            return a
        pad = a.new_zeros((a.shape[0], 1)) if torch.is_tensor(a) else np.zeros((a.shape[0], 1), np.float32)
        return torch.cat([a, pad], 1) if torch.is_tensor(a) else np.concatenate([a, pad], 1)

    if lengths is None:
        clouds = list(clouds)
        if not clouds:
            raise ValueError("no clouds")
        lengths = [int(c.shape[0]) for c in clouds]
        if all(torch.is_tensor(c) for c in clouds):
            packed = torch.cat([four(c.to(device, torch.float32)) for c in clouds], 0)
        else:
            host = [four(np.asarray(c.cpu() if torch.is_tensor(c) else c, dtype=np.float32)) for c in clouds]
            packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(host, 0)))
    else:
        lengths = [int(n) for n in lengths]
        packed = clouds if torch.is_tensor(clouds) else torch.from_numpy(np.ascontiguousarray(clouds, dtype=np.float32))
        packed = four(packed.to(torch.float32))
        if not lengths or min(lengths) < 0 or sum(lengths) != packed.shape[0]:
            raise ValueError(f"lengths sum to {sum(lengths)}, the packed tensor holds {packed.shape[0]} points")
    if sum(lengths) >= 2 ** 31 // 4:
        raise ValueError("the packed batch must stay below 2^31 floats")
    return packed.to(device).contiguous(), lengths


def project_scans(clouds, lengths=None, H=64, W=1024, fov_up=3.0, fov_down=-25.0, means=IMG_MEANS, stds=IMG_STDS, device="cuda"):
    """project_scan for a batch, on the device (rldm_rangenet_project): clouds as pack_clouds takes them -> ProjectedScans.
    A pixel goes to its nearest point and among equal depths to the lowest index (project_scan leaves that case to numpy's
    unstable argsort); a point whose depth is 0 or not finite is dropped (px = py = -1; the host code would index out of range).
    Nothing here waits for the device."""
    L = _lib.lib()
    dev = torch.device(device)
    pts, lengths = pack_clouds(clouds, lengths, dev)
    B, n = len(lengths), pts.shape[0]
    if B * 5 * H * W >= 2 ** 31:
        raise ValueError("the projected batch must stay below 2^31 elements")
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).to(dev)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    out = ProjectedScans(proj=new((B, 5, H, W), torch.float32), mask=new((B, H, W), torch.float32),
                         proj_range=new((B, H, W), torch.float32), proj_idx=new((B, H, W), torch.int32),
                         px=new((n,), torch.int32), py=new((n,), torch.int32), unproj_range=new((n,), torch.float32),
                         offsets=offsets, lengths=lengths, points=pts)
    keys = new((B, H, W), torch.int64)
    m5 = (C.c_float * 5)(*[float(v) for v in means])
    s5 = (C.c_float * 5)(*[float(v) for v in stds])
    with torch.cuda.device(dev):
        _lib.check(L.rldm_rangenet_project(_ptr(pts), _ptr(offsets), B, pts.shape[1], H, W, float(fov_up), float(fov_down), m5, s5,
                                           _ptr(keys), _ptr(out.proj), _ptr(out.mask), _ptr(out.proj_range), _ptr(out.proj_idx),
                                           _ptr(out.px), _ptr(out.py), _ptr(out.unproj_range), _lib.stream_ptr(dev)),
                   "rldm_rangenet_project")
    return out


def scatter_host(px, py, depth, points, remission=None, H=64, W=1024, means=IMG_MEANS, stds=IMG_STDS):
    """The device's pixel rule in numpy, given every point's pixel and depth: (proj (5, H, W), mask (H, W), proj_range (H, W),
    proj_idx (H, W) int32).  A lexsort on (pixel, depth, index) puts every pixel's winner first: the nearest point, the
    lowest index among equal depths.  Points with px < 0 take no part.  The normalisation and the mask are project_scan's
    expressions."""
    px, py = np.asarray(px).astype(np.int64).reshape(-1), np.asarray(py).astype(np.int64).reshape(-1)
    depth = np.asarray(depth, dtype=np.float32).reshape(-1)
    points = np.ascontiguousarray(points, dtype=np.float32)
    n = points.shape[0]
    remission = np.zeros(n, np.float32) if remission is None else np.asarray(remission, dtype=np.float32).reshape(-1)
    if not (px.shape[0] == py.shape[0] == depth.shape[0] == remission.shape[0] == n) or points.shape[1:] != (3,):
        raise ValueError("px, py, depth, points (N, 3) and remission must describe the same N points")
    valid = np.flatnonzero(px >= 0)
    pix = py[valid] * W + px[valid]
    order = np.lexsort((valid, depth[valid], pix))       # the last key is the primary one
    pix = pix[order]
    first = np.ones(pix.shape[0], bool)
    first[1:] = pix[1:] != pix[:-1]
    win, at = valid[order][first], pix[first]
    proj_range = np.full(H * W, -1, dtype=np.float32)
    proj_xyz = np.full((H * W, 3), -1, dtype=np.float32)
    proj_rem = np.full(H * W, -1, dtype=np.float32)
    proj_idx = np.full(H * W, -1, dtype=np.int32)
    proj_range[at], proj_xyz[at], proj_rem[at], proj_idx[at] = depth[win], points[win], remission[win], win
    proj_range, proj_rem, proj_idx = proj_range.reshape(H, W), proj_rem.reshape(H, W), proj_idx.reshape(H, W)
    mask = (proj_idx > 0).astype(np.float32)
    proj = np.concatenate([proj_range[None], proj_xyz.reshape(H, W, 3).transpose(2, 0, 1), proj_rem[None]], 0)
    proj = (proj - np.asarray(means, np.float32)[:, None, None]) / np.asarray(stds, np.float32)[:, None, None]
    return (proj * mask).astype(np.float32), mask, proj_range, proj_idx


# ---- back to the points: plain and KNN (postproc/KNN.py) -----------------------------------------------------------------
def knn_params(arch):
    """The `post.KNN.params` dict of an arch_cfg (knn, search, sigma, cutoff), checked."""
    params = arch.get("post", {}).get("KNN", {}).get("params")
    if not isinstance(params, dict) or any(k not in params for k in ("knn", "search", "sigma", "cutoff")):
        raise ValueError("the arch_cfg carries no post.KNN.params (knn, search, sigma, cutoff)")
    return check_knn({k: params[k] for k in ("knn", "search", "sigma", "cutoff")})


def check_knn(params):
    knn, search, sigma, cutoff = int(params["knn"]), int(params["search"]), float(params["sigma"]), float(params["cutoff"])
    if search % 2 == 0 or not 1 <= search <= 7:
        raise ValueError(f"KNN search must be odd and at most 7, got {search}")
    if not 1 <= knn <= search * search:
        raise ValueError(f"KNN knn must be in [1, search^2 = {search * search}], got {knn}")
    if not sigma > 0.0 or not cutoff >= 0.0:
        raise ValueError(f"KNN sigma must be positive and cutoff not negative, got {sigma} and {cutoff}")
    return {"knn": knn, "search": search, "sigma": sigma, "cutoff": cutoff}


def knn_weights(search, sigma):
    """(search^2,) float32: 1 - the normalised search x search Gaussian, computed in torch fp32 step by step as
    postproc/KNN.py's get_gaussian_kernel does, so that the bits are the reference's."""
    coord = torch.arange(search)
    gx = coord.repeat(search).view(search, search)
    grid = torch.stack([gx, gx.t()], dim=-1).float()
    mean, variance = (search - 1) / 2., sigma ** 2.
    g = (1. / (2. * math.pi * variance)) * torch.exp(-torch.sum((grid - mean) ** 2., dim=-1) / (2 * variance))
    g = g / torch.sum(g)
    return (1 - g).reshape(-1).numpy().astype(np.float32)


def knn_labels_host(proj_range, unproj_range, argmax, px, py, knn, search, sigma, cutoff, nclasses=NUM_CLASSES):
    """postproc/KNN.py forward in numpy for one scan: proj_range (H, W) fp32 (-1: empty), argmax (H, W) integer labels, and per
    point unproj_range, px, py -> (N,) uint8.  The window is search x search around (py, px) without azimuth wrap, entry
    k = dy * search + dx; outside the image range and label are 0 (F.unfold's padding); an in-image range < 0 becomes +inf; the
    centre's range is the point's own; distance = |entry - range| * knn_weights[k].  The knn smallest vote (a stable sort: ties
    go to the lowest k), beyond `cutoff` (if > 0) for nobody; the class in [1, nclasses) with the most votes wins, the lowest
    on ties, 1 without votes.  A point with px < 0 gets 0."""
    p = check_knn({"knn": knn, "search": search, "sigma": sigma, "cutoff": cutoff})
    knn, search = p["knn"], p["search"]
    proj_range = np.asarray(proj_range, dtype=np.float32)
    argmax = np.asarray(argmax).astype(np.int64)
    px, py = np.asarray(px).astype(np.int64).reshape(-1), np.asarray(py).astype(np.int64).reshape(-1)
    r = np.asarray(unproj_range, dtype=np.float32).reshape(-1)
    n, pad = r.shape[0], search // 2
    valid = px >= 0
    x, y = np.where(valid, px, 0), np.where(valid, py, 0)
    rp, lp = np.pad(proj_range, pad), np.pad(argmax, pad)            # zeros
    w = knn_weights(search, p["sigma"])
    dist = np.empty((n, search * search), np.float32)
    lab = np.empty((n, search * search), np.int64)
    for k in range(search * search):
        dy, dx = divmod(k, search)
        e = rp[y + dy, x + dx]
        e = np.where(e < 0, np.float32(np.inf), e)
        if k == (search * search - 1) // 2:
            e = r
        dist[:, k] = np.abs(e - r) * w[k]
        lab[:, k] = lp[y + dy, x + dx]
    order = np.argsort(dist, axis=1, kind="stable")[:, :knn]
    near_d, near_l = np.take_along_axis(dist, order, 1), np.take_along_axis(lab, order, 1)
    if p["cutoff"] > 0:
        near_l = np.where(near_d > np.float32(p["cutoff"]), nclasses, near_l)
    votes = np.zeros((n, nclasses + 1), np.int64)
    np.add.at(votes, (np.repeat(np.arange(n), knn), np.minimum(near_l, nclasses).reshape(-1)), 1)
    out = votes[:, 1:-1].argmax(axis=1) + 1
    return np.where(valid, out, 0).astype(np.uint8)


def unproject(scans, argmax, knn=None, num_classes=NUM_CLASSES):
    """Per-point labels of a ProjectedScans batch from the network's argmax (uint8 (B, H, W), device): uint8 (sum N,) on the
    device (rldm_rangenet_unproject).  knn None: argmax[py, px]; a params dict (knn_params): the KNN vote.  Does not wait."""
    L = _lib.lib()
    dev = scans.proj_range.device
    B, H, W = scans.proj_range.shape
    if tuple(argmax.shape) != (B, H, W) or argmax.dtype != torch.uint8 or argmax.device != dev:
        raise ValueError(f"argmax must be uint8 {(B, H, W)} on {dev}")
    argmax = argmax.contiguous()
    labels = torch.empty((scans.px.shape[0],), dtype=torch.uint8, device=dev)
    k = search = 0
    cutoff, weights = 0.0, None
    if knn is not None:
        k, search, cutoff = int(knn["knn"]), int(knn["search"]), float(knn["cutoff"])
        if k < 1:
            raise ValueError(f"KNN knn must be at least 1, got {k}")
        weights = torch.from_numpy(knn_weights(search, float(knn["sigma"])) if search >= 1 else np.zeros(1, np.float32)).to(dev)
    with torch.cuda.device(dev):
        _lib.check(L.rldm_rangenet_unproject(_ptr(scans.proj_range), _ptr(argmax), _ptr(scans.px), _ptr(scans.py),
                                             _ptr(scans.unproj_range), _ptr(scans.offsets), B, H, W, k, search, _ptr(weights),
                                             cutoff, int(num_classes), _ptr(labels), _lib.stream_ptr(dev)), "rldm_rangenet_unproject")
    return labels


# ---- segmentation agreement ----------------------------------------------------------------------------------------------
def confusion_matrix(pred, target, num_classes=NUM_CLASSES):
    """(num_classes, num_classes) int64 counts [target][pred], by integer counting on the tensors' device (torch.bincount)."""
    pred, target = torch.as_tensor(pred), torch.as_tensor(target)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    p, t = pred.reshape(-1).to(torch.int64), target.reshape(-1).to(torch.int64)
    if p.numel() == 0:
        raise ValueError("empty segmentation")
    if int(torch.min(p.min(), t.min())) < 0 or int(torch.max(p.max(), t.max())) >= num_classes:
        raise ValueError(f"labels outside [0, {num_classes})")
    return torch.bincount(t * num_classes + p, minlength=num_classes * num_classes).reshape(num_classes, num_classes)


def scores_from_confusion(cm):
    """{"accuracy", "iou"} of a [target][pred] count matrix: accuracy = trace / total; iou = sklearn's
    jaccard_score(target, pred, average="weighted"): per class TP / (TP + FP + FN) over the labels present in either input,
    weighted by the class's support in `target`."""
    cm = np.asarray(torch.as_tensor(cm).cpu(), dtype=np.int64)
    tp = np.diag(cm)
    support, predicted = cm.sum(1), cm.sum(0)
    union = support + predicted - tp
    present = union > 0
    iou = tp[present] / union[present].astype(np.float64)
    total = int(cm.sum())
    return {"accuracy": float(tp.sum() / float(total)), "iou": float((iou * support[present]).sum() / float(support.sum()))}


def segmentation_scores(pred, target, num_classes=NUM_CLASSES):
    """metrics/metrics/iou.py: calculate_accuracy and calculate_iou of two label tensors of one shape."""
    return scores_from_confusion(confusion_matrix(pred, target, num_classes))


# ---- the device network --------------------------------------------------------------------------------------------------
def kernel_weight(kind, w):
    """The reference's weight tensor as rldm_rangenet_pack_weights takes it: fp32 (Cout, T, Cin) contiguous numpy."""
    w = torch.as_tensor(w).detach().to("cpu", torch.float32)
    if kind == KIND_UPCONV:
        w = w[:, :, 0, :].permute(1, 2, 0)               # (Cin, Cout, 4) -> (Cout, 4, Cin)
    else:
        w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1])
    return np.ascontiguousarray(w.numpy(), dtype=np.float32)


def pack_weights(kind, w, device="cuda"):
    """Device int16 tensor: the packed bf16 weight image of one layer (w in the reference's layout)."""
    L = _lib.lib()
    kw = kernel_weight(kind, w)
    cout, _, cin = kw.shape
    n = int(L.rldm_rangenet_packed_elems(kind, cin, cout))
    packed = np.empty(n, np.uint16)
    _lib.check(L.rldm_rangenet_pack_weights(kind, cin, cout, kw.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)),
               "rldm_rangenet_pack_weights")
    return torch.from_numpy(packed.view(np.int16)).to(device)


def to_device_layout(x, device="cuda"):
    """fp32 (B, C, H, W) -> device bf16 [B][H][W][pitch(C)], zero padded (torch rounds to nearest even, as the kernel does)."""
    B, Cc, H, W = x.shape
    out = torch.zeros((B, H, W, pitch(Cc)), dtype=torch.bfloat16, device=device)
    out[..., :Cc] = x.to(device).permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def from_device_layout(y, channels):
    """device bf16 [B][H][W][pitch] -> fp32 (B, channels, H, W) on the host."""
    return y[..., :channels].permute(0, 3, 1, 2).to(torch.float32).cpu()


def gather_map(indices, total, device="cuda"):
    """(mask, slot) of rldm_rangenet_layer's gather: mask int32 words with bit i & 31 of word i >> 5 set for every gathered
    position i of one image's flattened feature map, slot int32 (total,) with slot[i] = the column position i is written to.
    The indices must be distinct (frd_indices draws without replacement)."""
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=device)
    if idx.ndim != 1 or idx.numel() == 0:
        raise ValueError("gather must be a non-empty list of indices")
    if int(idx.min()) < 0 or int(idx.max()) >= total:
        raise ValueError(f"gather index outside [0, {total})")
    if int(torch.unique(idx).numel()) != int(idx.numel()):
        raise ValueError("gather indices must be distinct")
    words = torch.zeros((total + 31) // 32, dtype=torch.int64, device=device)
    words.index_add_(0, idx >> 5, torch.ones_like(idx) << (idx & 31))     # distinct bits: the sum is the OR
    slot = torch.zeros(total, dtype=torch.int32, device=device)
    slot[idx] = torch.arange(idx.numel(), dtype=torch.int32, device=device)
    return words.to(torch.int32), slot                   # (int64 -> int32 keeps the low 32 bits)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run_layer(kind, x, w_packed, scale, shift, cin, cout, leaky=True, add0=None, add1=None, want_f32=False, gather=None,
              want_argmax=False):
    """rldm_rangenet_layer on device tensors: x bf16 [B][H][W][pitch(cin)], w_packed from pack_weights, scale / shift fp32
    (cout,), add0 / add1 bf16 of the output's layout -> dict with `out` (bf16 [B][H][W_out][pitch(cout)]) and, as asked,
    `f32` (B, cout, H, W_out), `gathered` (B, len(gather)), `argmax` uint8 (B, H, W_out)."""
    L = _lib.lib()
    B, H, W, cp = x.shape
    if cp != pitch(cin) or x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise ValueError(f"x must be contiguous bf16 [B][H][W][{pitch(cin)}]")
    Wout = (W - 1) // 2 + 1 if kind == KIND_3X3_S2 else 2 * W if kind == KIND_UPCONV else W
    dev = x.device
    res = {"out": torch.empty((B, H, Wout, pitch(cout)), dtype=torch.bfloat16, device=dev)}
    for name, add in (("add0", add0), ("add1", add1)):
        if add is not None and (tuple(add.shape) != tuple(res["out"].shape) or add.dtype != torch.bfloat16 or not add.is_contiguous()):
            raise ValueError(f"{name} must be contiguous bf16 of shape {tuple(res['out'].shape)}")
    if want_f32:
        res["f32"] = torch.empty((B, cout, H, Wout), dtype=torch.float32, device=dev)
    mask = slot = None
    n_gather = 0
    if gather is not None:
        mask, slot = gather_map(gather, cout * H * Wout, dev)
        n_gather = len(gather)
        res["gathered"] = torch.empty((B, n_gather), dtype=torch.float32, device=dev)
    if want_argmax:
        res["argmax"] = torch.empty((B, H, Wout), dtype=torch.uint8, device=dev)
    scale = scale.to(dev, torch.float32).contiguous()
    shift = shift.to(dev, torch.float32).contiguous()
    if scale.numel() != cout or shift.numel() != cout:
        raise ValueError(f"scale / shift must hold {cout} values")
    d = _lib.RangeNetLayerDescC(kind, B, H, W, cin, cout, int(bool(leaky)))
    _lib.check(L.rldm_rangenet_layer(C.byref(d), _ptr(x), _ptr(w_packed), _ptr(scale), _ptr(shift), _ptr(add0), _ptr(add1),
                                     _ptr(res["out"]), _ptr(res.get("f32")), _ptr(mask), _ptr(slot), n_gather,
                                     _ptr(res.get("gathered")), _ptr(res.get("argmax")), _lib.stream_ptr(dev)),
               "rldm_rangenet_layer")
    return res


class RangeNet:
    """DarkNet21 / DarkNet53 RangeNet++ on the GPU.  Not thread-safe: one forward per object at a time (the library object owns
    its activation arena)."""

    def __init__(self, state, device="cuda"):
        _lib.require_gpu()
        L = _lib.lib()
        self.state = state
        self.layers = state["layers"]
        self.device = torch.device(device)
        self._cfg = _lib.RangeNetConfigC(self.layers, 5, NUM_CLASSES)
        specs = state["specs"]
        n = int(L.rldm_rangenet_num_layers(C.byref(self._cfg)))
        if n != len(specs):
            raise RuntimeError(f"librangeldm_hip walks {n} layers, the state holds {len(specs)}")
        info = _lib.RangeNetLayerDescC()
        for i, s in enumerate(specs):                    # the library's walk and this module's must agree layer by layer
            _lib.check(L.rldm_rangenet_layer_info(C.byref(self._cfg), i, C.byref(info)), "rldm_rangenet_layer_info")
            if (info.kind, info.Cin, info.Cout, info.leaky) != (s["kind"], s["cin"], s["cout"], int(s["leaky"])):
                raise RuntimeError(f"layer {i}: the library expects kind {info.kind} {info.Cin}->{info.Cout}")
        ws = [kernel_weight(s["kind"], s["w"]) for s in specs]
        scs = [np.ascontiguousarray(s["scale"].numpy(), dtype=np.float32) for s in specs]
        shs = [np.ascontiguousarray(s["shift"].numpy(), dtype=np.float32) for s in specs]
        arr = lambda xs: (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.rldm_rangenet_create(C.byref(self._cfg), arr(ws), arr(scs), arr(shs), len(specs), C.byref(self._h)),
                       "rldm_rangenet_create")
        self._gather_key, self._gather = None, None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib().rldm_rangenet_destroy(h)
            self._h = None

    @classmethod
    def from_state(cls, arch, backbone_sd, decoder_sd, head_sd, device="cuda"):
        return cls(fold_state(arch, backbone_sd, decoder_sd, head_sd), device)

    @classmethod
    def from_pretrained(cls, model_dir, device="cuda"):
        """model_dir: arch_cfg.yaml and the torch-saved `backbone`, `segmentation_decoder`, `segmentation_head` state dicts."""
        arch, sds = load_pretrained(model_dir)
        return cls.from_state(arch, *sds, device=device)

    def _forward(self, proj, gather, want_features, want_argmax, want_logits):
        L = _lib.lib()
        if proj.ndim != 4 or proj.shape[1] != 5:
            raise ValueError(f"proj must be (B, 5, H, W), got {tuple(proj.shape)}")
        proj = proj.to(self.device, torch.float32).contiguous()
        B, _, H, W = proj.shape
        if W % 32:
            raise ValueError(f"the width must be a multiple of 32 (five halvings), got {W}")
        mask = slot = features = argmax = logits = None
        n_gather = 0
        if gather is not None:
            key = (H, W, tuple(int(i) for i in gather))
            if key != self._gather_key:
                self._gather_key, self._gather = key, gather_map(gather, FEATURE_CHANNELS * H * W, self.device)
            mask, slot = self._gather
            n_gather = len(key[2])
            features = torch.empty((B, n_gather), dtype=torch.float32, device=self.device)
        elif want_features:
            features = torch.empty((B, FEATURE_CHANNELS, H, W), dtype=torch.float32, device=self.device)
        if want_argmax:
            argmax = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        if want_logits:
            logits = torch.empty((B, NUM_CLASSES, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.rldm_rangenet_forward(self._h, _ptr(proj), B, H, W, _ptr(mask), _ptr(slot), n_gather, _ptr(features),
                                               _ptr(argmax), _ptr(logits), _lib.stream_ptr(self.device)), "rldm_rangenet_forward")
        return argmax, features, logits

    def infer(self, proj, gather=None):
        """proj (B, 5, H, W) fp32 -> (argmax uint8 (B, H, W), features): fp32 (B, 32, H, W), or (B, len(gather)) = the values
        at `gather` (distinct indices into one scan's `reshape(-1)` of (32, H, W), metrics.frd_indices) when a list is given."""
        argmax, features, _ = self._forward(proj, gather, True, True, False)
        return argmax, features

    def logits(self, proj):
        """fp32 (B, 20, H, W): the head's output before the softmax (tests)."""
        return self._forward(proj, None, False, False, True)[2]

    def segment(self, clouds, knn=None, H=64, W=1024, lengths=None):
        """Per-point labels of a batch of scans (clouds as pack_clouds takes them): a list of uint8 arrays, one per cloud.
        Projection, forward and unprojection run on the device; the host waits once, for the labels.  knn: a params dict
        (knn_params(arch)) for the reference's KNN clean-up, None for the plain `argmax[py, px]`."""
        scans = project_scans(clouds, lengths, H=H, W=W, device=self.device)
        argmax, _, _ = self._forward(scans.proj, None, False, True, False)
        labels = unproject(scans, argmax, knn).cpu().numpy()
        return [part.copy() for part in np.split(labels, np.cumsum(scans.lengths)[:-1])]


def load_pretrained(model_dir):
    """(arch, (backbone_sd, decoder_sd, head_sd)) of a model folder in the layout of the reference's darknet53-1024/.  The
    architecture is checked before a weight file is read."""
    import yaml
    with open(os.path.join(model_dir, "arch_cfg.yaml")) as f:
        arch = yaml.safe_load(f)
    check_arch(arch)
    sds = tuple(torch.load(os.path.join(model_dir, name), map_location="cpu", weights_only=True)
                for name in ("backbone", "segmentation_decoder", "segmentation_head"))
    return arch, sds


def save_pretrained(model_dir, arch, backbone_sd, decoder_sd, head_sd):
    """Write a model folder load_pretrained reads (tests and tools: a synthetic network on disk)."""
    import yaml
    os.makedirs(model_dir, exist_ok=True)
    with open(os.path.join(model_dir, "arch_cfg.yaml"), "w") as f:
        yaml.safe_dump(arch, f)
    for name, sd in (("backbone", backbone_sd), ("segmentation_decoder", decoder_sd), ("segmentation_head", head_sd)):
        torch.save(dict(sd), os.path.join(model_dir, name))


def synthetic_cloud(seed, n=60000):
    """A seeded LiDAR-like scan: (points (n, 3), remission (n,)) float32 with pairwise distinct depths -- a flat ground plane,
    a ring of walls and scattered boxes seen from a 64-beam sensor 1.73 m above the ground (tests, tools)."""
    u = synth.uniform(seed, "rangenet/cloud", (n, 4)).astype(np.float64) * 0.5 + 0.5
    yaw = (u[:, 0] * 2.0 - 1.0) * np.pi
    pitch_ = np.deg2rad(-24.8 + 27.6 * u[:, 1])
    wall = 12.0 + 8.0 * np.sin(3.0 * yaw) + 4.0 * np.sin(7.0 * yaw + 1.0)
    ground = np.where(pitch_ < -0.01, 1.73 / np.maximum(np.sin(-pitch_), 1e-3), 1e9)
    depth = np.minimum(np.minimum(wall, ground), 60.0) * (1.0 + 0.01 * (u[:, 2] - 0.5))
    pts = np.stack([depth * np.cos(pitch_) * np.cos(yaw), depth * np.cos(pitch_) * np.sin(yaw), depth * np.sin(pitch_)], 1)
    pts = pts.astype(np.float32)
    d32 = np.linalg.norm(pts, 2, axis=1)
    _, first = np.unique(d32, return_index=True)         # drop the (rare) fp32 depth ties: argsort leaves their order undefined
    keep = np.sort(first)
    return pts[keep], (u[keep, 3] * 0.6).astype(np.float32)
