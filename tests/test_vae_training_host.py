"""CPU: the host side of VAE decoder fine-tuning -- the numpy statement of the L1 loss's fixed summation order (train_ops.l1_host), the
trainer's parameter plan (rangeldm_amd/vae_training.py), the command line of rangeldm_amd.train_vae and the vae/ directory it writes."""
import json
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import train_ops as T
from rangeldm_amd import train_vae as CLI
from rangeldm_amd import vae_training as VT
from rangeldm_amd.config import UNetConfig, VAEConfig
from rangeldm_amd.params import unet_param_shapes, vae_param_shapes
from rangeldm_amd.synth import synth_state_dict

SMALL = VAEConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, sample_size=(32, 8))


def _data(B, Cc, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, W, H, Cc, generator=g)
    target = torch.randn(B, Cc, W, H, generator=g)
    return pred, target


def _tree(v):
    """A 256-value block added as train_common.h's block_sum_d adds it, one scalar operation at a time: per 64-lane wave lane l with
    l ^ 32, then ^ 16 .. ^ 1; then the four waves in order from 0."""
    assert len(v) == 256
    acc = np.float64(0.0)
    for w in range(4):
        lanes = [np.float64(x) for x in v[64 * w:64 * w + 64]]
        o = 32
        while o:
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
            o >>= 1
        acc = acc + lanes[0]
    return acc


def _ordered_total(values):
    """mse's deterministic order, restated with scalar loops: partial i = _tree of elements [256 i, 256 i + 256) (zeros past the end);
    thread t of 256 adds partials t, t + 256, ... in order; _tree over the 256 threads."""
    v = np.asarray(values, np.float64).reshape(-1)
    nb = (v.size + 255) // 256
    v = np.concatenate([v, np.zeros(nb * 256 - v.size)])
    parts = [_tree(v[256 * i:256 * i + 256]) for i in range(nb)]
    threads = []
    for t in range(256):
        a = np.float64(0.0)
        for i in range(t, nb, 256):
            a = a + parts[i]
        threads.append(a)
    return _tree(threads)


@pytest.mark.parametrize("shape,wc", [((2, 2, 8, 4), (40.0, 10.0)), ((3, 2, 5, 64), (40.0, 10.0)), ((1, 4, 7, 3), (1.5, 0.25, 3.0, 7.0)),
                                      ((5, 2, 32, 64), (40.0, 10.0))])
def test_l1_host_is_the_formula_in_the_stated_order(shape, wc):
    B, Cc, W, H = shape
    pred, target = _data(B, Cc, W, H, 11)
    loss, dpred, sums = T.l1_host(pred.numpy(), target.numpy(), wc)
    # the formula, torch fp64, on the fp32 differences
    d = (pred - target.permute(0, 2, 3, 1)).double()
    w = torch.tensor(wc, dtype=torch.float64)
    ref_loss = float((d.abs() * w).sum() / B)
    ref_sums = d.abs().sum((0, 1, 2))
    n = d.numel()
    assert abs(float(loss) - ref_loss) <= 4 * n * 2.0 ** -53 * ref_loss        # (any order of n fp64 additions)
    assert np.allclose(sums, ref_sums.numpy(), rtol=4 * n * 2.0 ** -53, atol=0)
    g32 = (torch.tensor(wc, dtype=torch.float32) / np.float32(B))
    assert np.array_equal(dpred, (torch.sign(d).float() * g32).numpy())
    assert dpred.dtype == np.float32 and np.asarray(loss).dtype == np.float64
    # the order: bit for bit the scalar restatement
    a = d.abs().numpy()
    contrib = (np.asarray(wc, np.float32).astype(np.float64) * a) / float(B)
    assert float(loss) == float(_ordered_total(contrib))
    for c in range(Cc):
        only = np.where(np.arange(Cc) == c, a, 0.0)
        assert float(sums[c]) == float(_ordered_total(only))


def test_l1_host_order_is_fixed_not_incidental():
    """The total is a function of which 256-element block an element sits in: the same multiset of contributions laid out in another
    element order gives (for data that spans many binades) other bits, and the stated order tracks it."""
    g = torch.Generator().manual_seed(3)
    mag = torch.exp2(torch.randint(-20, 20, (4, 16, 16, 2), generator=g).float())
    pred = mag * torch.randn(4, 16, 16, 2, generator=g)
    target = torch.zeros(4, 2, 16, 16)
    loss, _, _ = T.l1_host(pred.numpy(), target.numpy(), (40.0, 10.0))
    contrib = (np.array([40.0, 10.0]) * pred.abs().double().numpy()) / 4.0
    assert float(loss) == float(_ordered_total(contrib))
    rev = pred.flip(0, 1, 2)
    loss_rev, _, _ = T.l1_host(rev.numpy(), target.numpy(), (40.0, 10.0))
    assert float(loss_rev) == float(_ordered_total((np.array([40.0, 10.0]) * rev.abs().double().numpy()) / 4.0))
    assert abs(float(loss_rev) - float(loss)) <= 1e-12 * float(loss)


def test_l1_host_sign_of_zero_is_zero():
    pred, target = _data(2, 2, 4, 4, 5)
    tn = target.permute(0, 2, 3, 1)
    pred[0, 1, 2, 0] = tn[0, 1, 2, 0]
    pred[1, 3, 3, 1] = tn[1, 3, 3, 1]
    loss, dpred, sums = T.l1_host(pred.numpy(), target.numpy(), (40.0, 10.0))
    assert dpred[0, 1, 2, 0] == 0.0 and dpred[1, 3, 3, 1] == 0.0
    assert int((dpred == 0).sum()) == 2
    g = np.float32(40.0) / np.float32(2), np.float32(10.0) / np.float32(2)
    assert set(np.unique(dpred[..., 0])) == {-g[0], np.float32(0), g[0]} and set(np.unique(dpred[..., 1])) == {-g[1], np.float32(0), g[1]}


@pytest.mark.parametrize("cfg", [SMALL, VAEConfig(), VAEConfig(ch=64, ch_mult=(1, 2, 4), num_res_blocks=2, sample_size=(32, 64))])
def test_trainer_parameters_are_the_decoder_keys_in_tape_order(cfg):
    shapes = vae_param_shapes(cfg)
    names = VT.decoder_param_names(cfg)
    assert sorted(names) == sorted(k for k in shapes if k.startswith("decoder.")) and len(set(names)) == len(names)
    assert not any(n.startswith("encoder.") for n in names)
    # tape order: the layer sequence of oracle.vae.vae_decode; backward finishes the parameters in the reverse of this list
    layer_of = [n.rsplit(".", 1)[0] for n in names]
    layers = [l for i, l in enumerate(layer_of) if i == 0 or layer_of[i - 1] != l]
    assert len(layers) == len(set(layers)), "a layer's weight and bias are not adjacent"
    L = len(cfg.ch_mult)
    expect = ["decoder.conv_in"]
    chs = [cfg.ch * m for m in cfg.ch_mult]
    cin = chs[-1]

    def resnet(p, cin, cout):
        return [p + ".norm1", p + ".conv1", p + ".norm2"] + ([p + ".conv_shortcut"] if cin != cout else []) + [p + ".conv2"]
    expect += resnet("decoder.mid_block.resnets.0", cin, cin) + resnet("decoder.mid_block.resnets.1", cin, cin)
    for i in range(L):
        cout = chs[L - 1 - i]
        for j in range(cfg.num_res_blocks + 1):
            expect += resnet(f"decoder.up_blocks.{i}.resnets.{j}", cin, cout)
            cin = cout
        if i != L - 1:
            expect.append(f"decoder.up_blocks.{i}.upsamplers.0.conv")
    expect += ["decoder.conv_norm_out", "decoder.conv_out"]
    assert layers == expect


def test_cli_arguments_and_log_line():
    a = CLI.build_parser().parse_args(["--weights", "w", "--input", "in", "--out", "o", "--steps", "7"])
    assert (a.weights, a.input, a.out, a.steps, a.batch_size, a.lr, a.mode, a.log_every) == ("w", "in", "o", 7, 8, 4.5e-6, False, 10)
    assert a.sgm_ckpt is None and a.sgm_yaml is None and a.deterministic is False
    CLI.check_args(a)
    b = CLI.build_parser().parse_args(["--sgm-ckpt", "f.ckpt", "--sgm-yaml", "y.yaml", "--out", "o", "--steps", "2", "--batch-size", "4",
                                       "--lr", "1e-5", "--mode", "--seed", "9", "--log-every", "1"])
    assert (b.sgm_ckpt, b.sgm_yaml, b.batch_size, b.lr, b.mode, b.seed, b.log_every, b.input) == ("f.ckpt", "y.yaml", 4, 1e-5, True, 9, 1, None)
    CLI.check_args(b)
    with pytest.raises(SystemExit):
        CLI.build_parser().parse_args(["--steps", "3"])                      # --out is required
    for bad in (["--out", "o", "--steps", "0"], ["--out", "o", "--steps", "1", "--weights", "w", "--sgm-ckpt", "c"],
                ["--out", "o", "--steps", "1", "--sgm-yaml", "y"], ["--out", "o", "--steps", "1", "--log-every", "0"]):
        with pytest.raises(ValueError):
            CLI.check_args(CLI.build_parser().parse_args(bad))
    rec = json.loads(json.dumps(CLI.log_record(20, np.float64(3.5), [1024.0, 256.0], 8 * 16 * 4)))
    assert rec == {"step": 20, "loss": 3.5, "mae": [2.0, 0.5]}
    files = [f"{i}.npy" for i in range(5)]
    assert CLI.batch_files(files, 0, 2) == ["0.npy", "1.npy"] and CLI.batch_files(files, 2, 2) == ["4.npy", "0.npy"]


def test_saved_vae_directory_round_trips(tmp_path):
    """What save_pretrained writes (save_vae_dir over the merged state dict) is what load_output_dir / `evaluate vae --weights` read."""
    from rangeldm_amd import checkpoint as ck
    sd = synth_state_dict(vae_param_shapes(SMALL), prefix="vt.")
    trained = {k: v + 1.0 for k, v in sd.items() if k.startswith("decoder.")}
    merged = VT.merged_state_dict(sd, trained)
    assert list(merged) != [] and set(merged) == set(sd)
    out = str(tmp_path / "run")
    VT.save_vae_dir(out, SMALL, merged)
    ucfg = UNetConfig(sample_size=(16, 4), block_out_channels=(32, 32, 64, 64))
    ck.save_model_dir(os.path.join(out, "unet"), ck.unet_config_to_diffusers(ucfg), synth_state_dict(unet_param_shapes(ucfg), prefix="u."))
    got = ck.load_output_dir(out)
    assert got["vae_config"] == SMALL
    assert set(got["vae"]) == set(sd)
    for k, v in sd.items():
        assert tuple(got["vae"][k].shape) == tuple(v.shape)
        want = trained[k] if k.startswith("decoder.") else v
        assert np.array_equal(np.asarray(got["vae"][k]), want), k
