"""bench.py `--dump-outputs` on the host: what is written, the size cap with its fixed sample, and the argument checks that run
before any device is touched."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_npy(tmp_path):
    x = torch.randn(4, 2, 16, 8, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"images": x})
    assert sorted(os.listdir(tmp_path / "d")) == ["images.npy"]
    a = np.load(tmp_path / "d" / "images.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())


def test_dump_outputs_caps_the_total_with_a_fixed_sample_of_images(tmp_path):
    n = 300                                                  # 300 images of 2 x 1024 x 64 fp32: 157 MB, over the cap
    x = torch.arange(n, dtype=torch.float32)[:, None, None, None].expand(n, 2, 1024, 64)   # image i holds the value i
    bench.dump_outputs(str(tmp_path / "a"), {"images": x})
    bench.dump_outputs(str(tmp_path / "b"), {"images": x})
    a, b = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert a.nbytes <= bench.DUMP_LIMIT_BYTES and a.shape == (bench.DUMP_LIMIT_BYTES // (2 * 1024 * 64 * 4), 2, 1024, 64)
    rows = a[:, 0, 0, 0].astype(np.int64)
    assert (a == rows[:, None, None, None]).all()            # whole images, unaltered
    assert (np.diff(rows) > 0).all() and rows[-1] < n        # distinct images, in their original order
    assert np.array_equal(a, b)                              # the same sample every run


def _bench_args(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300,
                          cwd=ROOT)


def test_bench_rejects_zero_timed_steps():
    r = _bench_args("--gpus", "1", "--steps", "0", "--warmup", "1")
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_rejects_dump_outputs_with_train(tmp_path):
    r = _bench_args("--train", "--dump-outputs", str(tmp_path / "d"))
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()
