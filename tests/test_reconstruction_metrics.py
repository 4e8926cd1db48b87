"""Reconstruction metrics: range-image errors, beam-upsampling baselines, the VAE round trip and the evaluate driver
(rangeldm_amd/csrc/chamfer.hip, rangeldm_amd/evaluate.py; ldm/convert_vae.py:193-271, metrics/metrics/mae.py:45-117).

CPU: the driver's argument parsing and file pairing, the cubic-weight restatement, the refusals (nuScenes, log sensors).
GPU: range_errors against an fp64 numpy restatement, both beam_upsample modes bit-equal to numpy restatements (also past
the 4 194 304 outputs that one pass of the kernel's capped grid of 256 * 64 workgroups covers), `vae(x)` against encode -> mode -> decode, and `evaluate densification` end to end on inference_conditional's output.
"""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from rangeldm_amd import evaluate as E
from rangeldm_amd import metrics as M


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_parser_reads_every_command():
    p = E.build_parser()
    a = p.parse_args(["vae", "--weights", "w", "--samples", "8", "--batch-size", "2", "--json", "o.json"])
    assert (a.cmd, a.weights, a.samples, a.batch_size, a.json, a.input) == ("vae", "w", 8, 2, "o.json", None)
    a = p.parse_args(["vae", "--sgm-ckpt", "m.ckpt", "--sgm-yaml", "m.yaml"])
    assert (a.sgm_ckpt, a.sgm_yaml, a.samples, a.batch_size) == ("m.ckpt", "m.yaml", 1000, 4)
    a = p.parse_args(["densification", "--exp", "e"])
    assert (a.cmd, a.exp, a.cfg) == ("densification", "e", "upsample")
    a = p.parse_args(["inpainting", "--exp", "e", "--cfg", "x.yaml"])
    assert (a.cmd, a.cfg) == ("inpainting", "x.yaml")
    a = p.parse_args(["chamfer", "A", "B", "--columns", "3"])
    assert (a.a_dir, a.b_dir, a.columns) == ("A", "B", 3)
    with pytest.raises(SystemExit):
        p.parse_args(["densification"])                 # --exp is required
    with pytest.raises(SystemExit):
        p.parse_args([])


def _touch(path):
    np.zeros((2, 4), np.float32).tofile(path)


def test_result_files_pair_with_their_seed0_target(tmp_path):
    res, tgt = tmp_path / "densification_result", tmp_path / "densification_target"
    res.mkdir()
    tgt.mkdir()
    for j in range(3):
        _touch(tgt / f"{j}_seed_0.bin")
        for s in (0, 1, 5):
            _touch(res / f"{j}_seed_{s}.bin")
    (res / "0_seed_0.png").write_bytes(b"")
    (res / "notes.bin").write_bytes(b"")
    pairs = E.pair_result_files(str(res), str(tgt))
    assert len(pairs) == 9
    names = [(os.path.basename(r), os.path.basename(t)) for r, t in pairs]
    assert names[:3] == [("0_seed_0.bin", "0_seed_0.bin"), ("0_seed_1.bin", "0_seed_0.bin"), ("0_seed_5.bin", "0_seed_0.bin")]
    assert all(t == f"{r.split('_')[0]}_seed_0.bin" for r, t in names)
    _touch(res / "7_seed_2.bin")
    with pytest.raises(FileNotFoundError, match="no target"):
        E.pair_result_files(str(res), str(tgt))
    with pytest.raises(FileNotFoundError):
        E.pair_result_files(str(tgt / "missing"), str(tgt))


def test_chamfer_folders_pair_by_name(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    for n in ("0.bin", "1.bin", "2.bin"):
        _touch(a / n)
    for n in ("1.bin", "2.bin", "3.bin"):
        _touch(b / n)
    assert [os.path.basename(x) for x, _ in E.pair_by_name(str(a), str(b))] == ["1.bin", "2.bin"]


def test_cubic_weights_restatement():
    w = M.cubic_weights(0.0)
    assert w.dtype == np.float32 and w.tolist() == [0.0, 1.0, 0.0, 0.0]      # frac 0 reproduces the source row
    fr = np.linspace(0, 1, 257, dtype=np.float32)
    ws = M.cubic_weights(fr)
    assert np.all(np.abs(ws.astype(np.float64).sum(1) - 1.0) <= 1e-6)
    # Keys' kernel at A = -0.75, written out in fp64 at the same points
    A, x = -0.75, fr.astype(np.float64)

    def k(t):
        t = np.abs(t)
        return np.where(t <= 1, (A + 2) * t ** 3 - (A + 3) * t ** 2 + 1,
                        np.where(t < 2, A * t ** 3 - 5 * A * t ** 2 + 8 * A * t - 4 * A, 0.0))
    ref = np.stack([k(x + 1), k(x), k(1 - x), k(2 - x)], 1)
    assert np.max(np.abs(ws - ref)) < 1e-6
    assert M.cubic_weights(0.5).tolist() == M.cubic_weights(0.5)[::-1].tolist()   # symmetric at the midpoint


def test_evaluate_refuses_nuscenes_and_log_sensors():
    from rangeldm_amd.inference import sensor_for
    from rangeldm_amd.range_image import point_cloud_to_range_image_KITTI
    with pytest.raises(NotImplementedError, match="ring"):
        E.require_reprojectable(sensor_for(32))
    assert E.require_reprojectable(sensor_for(64)) is not None
    with pytest.raises(NotImplementedError, match="linear"):
        E.range_affine(point_cloud_to_range_image_KITTI(log=True))
    with pytest.raises(NotImplementedError, match="linear"):
        E.range_affine(point_cloud_to_range_image_KITTI(inverse=True))
    assert E.range_affine(point_cloud_to_range_image_KITTI()) == (40.0, 20.0)


def test_nuscenes_config_is_refused(tmp_path):
    cfg = tmp_path / "nus.yaml"
    cfg.write_text("all_circonv: true\nwith_vae: true\nupsample: 4\nresolution: [1024, 32]\nnuscenes: true\n")
    with pytest.raises(NotImplementedError, match="ring"):
        E.task_sensor(str(cfg))
    log = tmp_path / "log.yaml"
    log.write_text("all_circonv: true\nwith_vae: true\nupsample: 4\nresolution: [1024, 64]\nlog: true\n")
    _, sensor = E.task_sensor(str(log))
    with pytest.raises(NotImplementedError):
        E.range_affine(sensor)


def test_masked_window():
    assert E.masked_window(0.0625, 1024) == (0, 64)
    assert E.masked_window(0.25, 1024, start=0.875) == (896, 1024 + 128)      # wraps past the seam


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _ref_errors(a, b, scale, shift, channels, w0, w1):
    W = a.shape[2]
    cols = [(w0 + k) % W for k in range(w1 - w0)]
    s = np.asarray(scale, np.float64)[:, None, None]
    t = np.asarray(shift, np.float64)[:, None, None]
    sa, ss = [], []
    for i in range(a.shape[0]):
        d = ((a[i].astype(np.float64) * s + t) - (b[i].astype(np.float64) * s + t))[channels][:, cols]
        sa.append(np.abs(d).sum())
        ss.append((d * d).sum())
    return np.array(sa), np.array(ss), len(channels) * len(cols) * a.shape[3]


@pytest.mark.gpu
@pytest.mark.parametrize("channels,window", [(None, None), ([0], None), ([1], (60, 70)), ([0, 2], (5, 69))])
def test_range_errors_match_fp64(channels, window):
    rng = np.random.default_rng(1)
    a = rng.standard_normal((3, 3, 64, 16)).astype(np.float32)
    b = rng.standard_normal((3, 3, 64, 16)).astype(np.float32)
    scale, shift = [40.0, 1.0, 0.25], [20.0, 0.0, -3.0]
    sa, ss, n = M.range_errors(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), scale, shift, channels, window)
    ch = list(range(3)) if channels is None else channels
    w0, w1 = window or (0, 64)
    ra, rs, rn = _ref_errors(a, b, scale, shift, ch, w0, w1)
    assert n == rn
    assert np.allclose(sa.cpu().numpy(), ra, rtol=1e-12, atol=0)
    assert np.allclose(ss.cpu().numpy(), rs, rtol=1e-12, atol=0)


def _ref_upsample(src, rate, mode):
    Hs = src.shape[-1]
    r = np.arange(Hs * rate)
    if mode == "nearest":
        return src[..., r // rate]
    fy = ((r.astype(np.float64) + 0.5) * (1.0 / rate) - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    w = M.cubic_weights((fy - sy.astype(np.float32)).astype(np.float32))
    rows = [src[..., np.clip(sy - 1 + k, 0, Hs - 1)] for k in range(4)]
    return ((w[:, 0] * rows[0] + w[:, 1] * rows[1]) + w[:, 2] * rows[2]) + w[:, 3] * rows[3]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "bicubic"])
@pytest.mark.parametrize("rate", [4, 3])
def test_beam_upsample_matches_restatement(mode, rate):
    rng = np.random.default_rng(rate)
    src = rng.standard_normal((2, 2, 40, 16)).astype(np.float32)
    out = M.beam_upsample(torch.from_numpy(src).cuda(), rate, mode).cpu().numpy()
    ref = _ref_upsample(src, rate, mode).astype(np.float32)
    assert out.shape == (2, 2, 40, 16 * rate)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    if mode == "bicubic":                 # a constant image stays (nearly) constant: the weights sum to 1
        c = M.beam_upsample(torch.full((1, 1, 3, 8), 2.5, device="cuda"), rate, mode)
        assert float((c - 2.5).abs().max()) <= 1e-6


UPSAMPLE_GRID = 256 * 64 * 256                           # outputs one pass of beam_upsample_kernel's capped grid covers


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "bicubic"])
def test_beam_upsample_past_one_grid_matches_restatement(mode):
    """More than 4 194 304 outputs: the grid is capped at 256 * 64 workgroups and the first threads take a second trip."""
    rate = 4
    src = np.random.default_rng(5).standard_normal((1, 1, 65537, 16)).astype(np.float32)
    assert src.size * rate > UPSAMPLE_GRID
    out = M.beam_upsample(torch.from_numpy(src).cuda(), rate, mode).cpu().numpy()
    ref = _ref_upsample(src, rate, mode).astype(np.float32)
    assert out.shape == (1, 1, 65537, 16 * rate)
    bad = out.view(np.uint32) != ref.view(np.uint32)
    print(f"{mode}: {out.size} outputs, {out.size - UPSAMPLE_GRID} past one grid; {int(bad.sum())} differ "
          f"({int(bad.reshape(-1)[UPSAMPLE_GRID:].sum())} of those past one grid)")
    assert not bad.any()


def _small_vae():
    from rangeldm_amd.config import VAEConfig
    from rangeldm_amd.params import vae_param_shapes
    from rangeldm_amd.synth import synth_state_dict
    from rangeldm_amd.vae import AutoencoderKLHIP
    cfg = VAEConfig(sample_size=(128, 16))
    vae = AutoencoderKLHIP(cfg)
    vae.load_state_dict(synth_state_dict(vae_param_shapes(cfg), seed=3, prefix="vae."))
    return vae


@pytest.mark.gpu
def test_vae_call_is_encode_mode_decode():
    vae = _small_vae()
    x = torch.randn((2, 2, 128, 16), generator=torch.Generator().manual_seed(0)).cuda()
    out = vae(x)
    ref = vae.decode(vae.encode(x).latent_dist.mode()).sample
    assert torch.equal(out.sample, ref)
    (t,) = vae(x, return_dict=False)
    assert torch.equal(t, ref)
    s1 = vae(x, sample_posterior=True, generator=torch.Generator().manual_seed(4)).sample
    s2 = vae.decode(vae.encode(x).latent_dist.sample(generator=torch.Generator().manual_seed(4))).sample
    assert torch.equal(s1, s2) and not torch.equal(s1, ref)


@pytest.mark.gpu
def test_evaluate_densification_end_to_end(tmp_path):
    from rangeldm_amd import inference_conditional as IC
    exp = tmp_path / "exp"
    IC.main(["--cfg", "upsample", "--samples", "2", "--batch_size", "2", "--steps", "2", "--out", str(exp)])
    res = E.main(["densification", "--exp", str(exp), "--json", str(tmp_path / "d.json")])
    assert json.loads((tmp_path / "d.json").read_text()) == json.loads(json.dumps(res, sort_keys=True))
    # samples // batch + 1 = 2 seeds (ldm/inference_conditional.py:158) x 2 images
    assert res["task"] == "densification" and res["pairs"] == 4 and res["rate"] == 4
    assert set(res["mae_m"]) == set(res["cd"]) == {"ours", "nearest", "bicubic"}
    assert all(math.isfinite(v) and v >= 0 for d in (res["mae_m"], res["cd"]) for v in d.values())
    # target against itself: MAE 0 and CD 0
    same = tmp_path / "same"
    shutil.copytree(exp / "densification_target", same / "densification_result")
    shutil.copytree(exp / "densification_target", same / "densification_target")
    r0 = E.main(["densification", "--exp", str(same)])
    assert r0["mae_m"]["ours"] == 0.0 and r0["cd"]["ours"] == 0.0
    # the chamfer command on the same folders
    rc = E.main(["chamfer", str(exp / "densification_target"), str(exp / "densification_target")])
    assert rc["pairs"] == 2 and rc["cd"] == 0.0


@pytest.mark.gpu
def test_evaluate_vae_round_trip_runs():
    res = E.main(["vae", "--samples", "3", "--batch-size", "2"])
    assert res["task"] == "vae" and res["samples"] == 3 and res["weights"] == "synthetic"
    assert all(math.isfinite(res[k]) for k in ("mae", "psnr", "cd"))
