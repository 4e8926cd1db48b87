#!/usr/bin/env python3
"""Time what stands around the RangeNet++ forward (rangeldm_amd/csrc/rangenet_post.hip) on synthetic scans of about 120 000
points (rangenet.synthetic_cloud), batch 8, 64 x 1024; every figure is the median [min, max] of --reps repetitions after a
warm-up:

  host_project_scan          rangenet.project_scan, one scan (numpy: argsort + four scatters)
  host_knn_16_workers        rangenet.knn_labels_host over 16 scans in 16 forked workers, wall seconds per scan (run before this
                             process opens the GPU)
  device_project             rldm_rangenet_project on a packed batch already on the device: --inner calls, then one synchronise
  device_project_with_upload rangenet.project_scans from host arrays (pack, one upload, allocate, project), then synchronise
  device_knn                 rldm_rangenet_unproject, knn 5 / search 5 / sigma 1 / cutoff 1, the same way; and the plain mode
  frd_loop_host / _device    the inner loop of `evaluate frd --rangenet`: read --files .bin files, project (numpy, or one device
                             call per chunk of 8), forward DarkNet53 with the 4 096-value gather; scans per second

    python tools/bench_scan.py [--points 120000] [--batch 8] [--reps 5] [--inner 50] [--files 32] [--out FILE]

Time is a host clock around work that ends in a device synchronise.  The device labels and images are compared with the host
restatements on one scan before anything is timed.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

KNN = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
H, W = 64, 1024


def stats(ts, per=1):
    ts = [t / per for t in ts]
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "reps": len(ts)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def host_pixels(points):
    """project_scan's pixels (its lines before the sort)."""
    depth = np.linalg.norm(points, 2, axis=1)
    yaw = -np.arctan2(points[:, 1], points[:, 0])
    pitch = np.arcsin(points[:, 2] / depth)
    fd, fu = abs(-25.0 / 180.0 * np.pi), abs(3.0 / 180.0 * np.pi)
    fx = 0.5 * (yaw / np.pi + 1.0)
    fy = 1.0 - (pitch + fd) / (fd + fu)
    fx *= W
    fy *= H
    return (np.maximum(0, np.minimum(W - 1, np.floor(fx))).astype(np.int32),
            np.maximum(0, np.minimum(H - 1, np.floor(fy))).astype(np.int32), depth)


def _knn_job(job):
    from rangeldm_amd import rangenet as R
    proj_range, depth, labels, px, py = job
    t0 = time.perf_counter()
    out = R.knn_labels_host(proj_range, depth, labels, px, py, **KNN)
    return time.perf_counter() - t0, out


def host_knn(jobs, workers):
    import multiprocessing as mp
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_knn_job, [(j[0], j[1][:64], j[2], j[3][:64], j[4][:64]) for j in jobs[:workers]])        # start the workers
        t0 = time.perf_counter()
        res = pool.map(_knn_job, jobs, chunksize=1)
        wall = time.perf_counter() - t0
    return {"scans": len(jobs), "workers": workers, "wall_ms_per_scan": 1e3 * wall / len(jobs),
            "one_worker_ms_per_scan_median": 1e3 * float(np.median([r[0] for r in res]))}, res[0][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50, help="device calls per repetition (one synchronise at the end)")
    ap.add_argument("--files", type=int, default=32, help="clouds the frd loop reads per repetition")
    ap.add_argument("--layers", type=int, default=53)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rangeldm_amd import rangenet as R
    clouds = []
    for s in range(a.batch):
        pts, rem = R.synthetic_cloud(s, a.points)
        clouds.append(np.concatenate([pts, rem[:, None]], 1).astype(np.float32))
    out = {"points_per_scan": [int(c.shape[0]) for c in clouds], "batch": a.batch, "image": [H, W], "knn": KNN}

    # ---- host, before the GPU is opened (the KNN workers are forked) ----
    c0 = clouds[0]
    out["host_project_scan"] = stats(timed(lambda: R.project_scan(c0[:, :3], c0[:, 3]), a.reps))
    px, py, depth = host_pixels(c0[:, :3])
    _, _, proj_range, _ = R.scatter_host(px, py, depth, c0[:, :3], c0[:, 3], H, W)
    rng = np.random.default_rng(0)
    labels = np.repeat(np.repeat(rng.integers(0, R.NUM_CLASSES, (H // 4, W // 8)), 4, 0), 8, 1).astype(np.uint8)
    out["host_knn_16_workers"], _ = host_knn([(proj_range, depth, labels, px, py)] * 16, 16)
    print(json.dumps({k: out[k] for k in ("host_project_scan", "host_knn_16_workers")}), file=sys.stderr, flush=True)

    import ctypes as C
    import torch
    from rangeldm_amd import _lib
    from rangeldm_amd.metrics import frd_indices
    dev = torch.device("cuda")
    out["device"] = torch.cuda.get_device_name(0)
    L = _lib.lib()
    sync = torch.cuda.synchronize

    # ---- what is timed is what is tested: one scan against the host restatements ----
    s = R.project_scans(clouds, H=H, W=W)
    argmax = torch.from_numpy(np.broadcast_to(labels, (a.batch, H, W)).copy()).to(dev)
    n0 = clouds[0].shape[0]
    dpx, dpy, dr = (t[:n0].cpu().numpy() for t in (s.px, s.py, s.unproj_range))
    want = R.scatter_host(dpx, dpy, dr, c0[:, :3], c0[:, 3], H, W)
    out["image_equals_scatter_host"] = bool(all(np.array_equal(getattr(s, k)[0].cpu().numpy(), w)
                                                for k, w in zip(("proj", "mask", "proj_range", "proj_idx"), want)))
    out["pixels_differing_from_host"] = {"px": int((dpx != px).sum()), "py": int((dpy != py).sum()), "points": int(n0)}
    got = R.unproject(s, argmax, KNN)[:n0].cpu().numpy()
    out["knn_equals_knn_labels_host"] = bool(np.array_equal(got, R.knn_labels_host(want[2], dr, labels, dpx, dpy, **KNN)))

    # ---- device: the calls alone ----
    keys = torch.empty((a.batch, H, W), dtype=torch.int64, device=dev)
    m5, s5 = (C.c_float * 5)(*R.IMG_MEANS), (C.c_float * 5)(*R.IMG_STDS)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = _lib.stream_ptr(dev)

    def project_calls():
        for _ in range(a.inner):
            _lib.check(L.rldm_rangenet_project(p(s.points), p(s.offsets), a.batch, 4, H, W, 3.0, -25.0, m5, s5, p(keys), p(s.proj),
                                               p(s.mask), p(s.proj_range), p(s.proj_idx), p(s.px), p(s.py), p(s.unproj_range), st),
                       "rldm_rangenet_project")
        sync()
    ts = timed(project_calls, a.reps)
    total = sum(out["points_per_scan"])
    out["device_project"] = {"per_batch": stats(ts, a.inner), "per_scan": stats(ts, a.inner * a.batch)}
    # bytes the two kernels must move: 16 B read + 12 B written per point and one 8 B atomic; per pixel the key memset and read
    # (16 B), 16 B of the winner's point and 32 B of outputs
    need = total * (16 + 12 + 8) + a.batch * H * W * (16 + 16 + 32)
    out["device_project"]["bytes_needed"] = need
    out["device_project"]["gbytes_per_s"] = need / (1e6 * out["device_project"]["per_batch"]["median_ms"])

    def project_upload():
        R.project_scans(clouds, H=H, W=W)
        sync()
    out["device_project_with_upload"] = {"per_batch": stats(timed(project_upload, a.reps))}

    for name, params in (("device_knn", KNN), ("device_unproject_plain", None)):
        def calls():
            for _ in range(a.inner):
                R.unproject(s, argmax, params)
            sync()
        ts = timed(calls, a.reps)
        out[name] = {"per_batch": stats(ts, a.inner), "per_scan": stats(ts, a.inner * a.batch)}
    out["device_knn"]["speedup_vs_host_16_workers"] = out["host_knn_16_workers"]["wall_ms_per_scan"] / out["device_knn"]["per_scan"]["median_ms"]

    # ---- the inner loop of `evaluate frd --rangenet` ----
    from rangeldm_amd import evaluate as E
    arch = R.synthetic_arch(a.layers)
    net = R.RangeNet.from_state(arch, *R.synthetic_state(arch))
    idx = frd_indices()
    with tempfile.TemporaryDirectory() as d:
        files = []
        for i in range(a.files):
            files.append(os.path.join(d, f"{i:04d}.bin"))
            clouds[i % a.batch].tofile(files[-1])

        def forward_only():
            for _ in range(a.files // a.batch):
                net.infer(s.proj, gather=idx)
            sync()
        ts = timed(forward_only, a.reps)
        out["forward_with_gather"] = {"per_batch": stats(ts, a.files // a.batch), "layers": a.layers}
        for mode in ("host", "device"):
            def loop():
                for lo in range(0, len(files), a.batch):
                    net.infer(E._project_files(files[lo:lo + a.batch], dev, mode), gather=idx)
                sync()
            ts = timed(loop, a.reps)
            sps = [a.files / t for t in ts]
            out[f"frd_loop_{mode}"] = {"scans_per_s_median": float(np.median(sps)), "scans_per_s_min": min(sps),
                                       "scans_per_s_max": max(sps), "files": a.files, "reps": a.reps}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
