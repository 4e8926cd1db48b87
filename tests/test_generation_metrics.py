"""Set-level generation metrics (rangeldm_amd.metrics.generation_metrics / set_metrics / subsample, `evaluate generation`):
MMD-CD, COV-CD and 1-NNA-CD (Achlioptas et al. 2018; Yang et al. 2019) as reductions of the all-pairs Chamfer matrices, ties
decided by the lowest index.

CPU: argument errors before the device; subsample; the definitions restated in numpy (loops, below) and worked by hand on a
3 + 3 case with exact ties.
GPU: generation_metrics against the numpy restatement on a brute-force fp32 matrix (counts exactly, MMD within the summation
bound of tests/test_chamfer_matrix.py); planted sets with known answers; the evaluate driver, one process against two ranks.
"""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np_set_metrics(gg, gr, rr):
    """The definitions, one loop per sentence; `<` keeps the first minimum, i.e. the lowest index wins a tie."""
    gg, gr, rr = np.asarray(gg, np.float64), np.asarray(gr, np.float64), np.asarray(rr, np.float64)
    ng, nr = gr.shape
    # MMD: mean over reference clouds of the distance to the nearest generated cloud
    mmd = math.fsum(min(gr[g, r] for g in range(ng)) for r in range(nr)) / nr
    # COV: the reference clouds that are some generated cloud's nearest reference cloud
    covered = set()
    for g in range(ng):
        best = 0
        for r in range(1, nr):
            if gr[g, r] < gr[g, best]:
                best = r
        covered.add(best)
    # 1-NNA: nearest OTHER cloud in the union [G..., R...]; right when it carries the same label
    union = np.block([[gg, gr], [gr.T, rr]])
    right = []
    for a in range(ng + nr):
        best = None
        for b in range(ng + nr):
            if b != a and (best is None or union[a, b] < union[a, best]):
                best = b
        right.append((best >= ng) == (a >= ng))
    return {"mmd_cd": mmd, "cov_cd": len(covered) / nr, "nna_cd": sum(right) / (ng + nr), "nna_cd_gen": sum(right[:ng]) / ng,
            "nna_cd_ref": sum(right[ng:]) / nr, "n_gen": ng, "n_ref": nr}


# The hand-made case.  Rows of GR are generated clouds, columns reference clouds.
#   GR = [1 2 5]    column minima 1, 1, 2                      -> MMD = 4 / 3
#        [3 1 4]    row argmins: G0 -> R0, G1 -> R1, G2 -> R0 (2 = 2: a tie between R0 and R2, the lowest index wins)
#        [2 6 2]    covered = {R0, R1}                         -> COV = 2 / 3   (the other tie rule would give 3 / 3)
#   GG = [0 1 9]    RR = [0 7 1]    union rows without their diagonal:
#        [1 0 9]         [7 0 8]      G0: [. 1 9 | 1 2 5]  min 1 at G1 and R0: tie -> G1, same label   right
#        [9 9 0]         [1 8 0]      G1: [1 . 9 | 3 1 4]  min 1 at G0 and R1: tie -> G0               right
#                                     G2: [9 9 . | 2 6 2]  min 2 at R0                                 wrong
#                                     R0: [1 3 2 | . 7 1]  min 1 at G0 and R2: tie -> G0               wrong
#                                     R1: [2 1 6 | 7 . 8]  min 1 at G1                                 wrong
#                                     R2: [5 4 2 | 1 8 .]  min 1 at R0                                 right
#   -> 1-NNA = 3 / 6, over the generated clouds 2 / 3, over the reference clouds 1 / 3
HAND_GG = [[0, 1, 9], [1, 0, 9], [9, 9, 0]]
HAND_GR = [[1, 2, 5], [3, 1, 4], [2, 6, 2]]
HAND_RR = [[0, 7, 1], [7, 0, 8], [1, 8, 0]]
HAND_ANSWER = {"mmd_cd": 4 / 3, "cov_cd": 2 / 3, "nna_cd": 0.5, "nna_cd_gen": 2 / 3, "nna_cd_ref": 1 / 3, "n_gen": 3, "n_ref": 3}


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_hand_made_case_numpy_statements():
    assert _np_set_metrics(HAND_GG, HAND_GR, HAND_RR) == HAND_ANSWER
    assert M.set_metrics_host(HAND_GG, HAND_GR, HAND_RR) == HAND_ANSWER
    # a rectangular one: 2 generated, 3 reference.  GR = [4 4 9; 7 3 3]: G0 -> R0 (tie), G1 -> R1 (tie): COV 2 / 3,
    # MMD = (4 + 3 + 3) / 3; union rows: G0 [. 5 | 4 4 9] -> R0 wrong; G1 [5 . | 7 3 3] -> R1 wrong; R0 [4 7 | . 1 6] -> R1
    # right; R1 [4 3 | 1 . 2] -> R0 right; R2 [9 3 | 6 2 .] -> R1 right
    gg, gr, rr = [[0, 5], [5, 0]], [[4, 4, 9], [7, 3, 3]], [[0, 1, 6], [1, 0, 2], [6, 2, 0]]
    want = {"mmd_cd": 10 / 3, "cov_cd": 2 / 3, "nna_cd": 3 / 5, "nna_cd_gen": 0.0, "nna_cd_ref": 1.0, "n_gen": 2, "n_ref": 3}
    assert _np_set_metrics(gg, gr, rr) == want
    assert M.set_metrics_host(gg, gr, rr) == want


def test_argument_errors_come_before_the_device():
    good = torch.zeros((5, 3))
    with pytest.raises(ValueError, match="empty"):
        M.generation_metrics([good, torch.zeros((0, 3))], [good])
    with pytest.raises(ValueError, match="empty"):
        M.generation_metrics([good], [torch.zeros((0, 3)), good])
    with pytest.raises(ValueError, match="no point clouds"):
        M.generation_metrics([], [good])
    with pytest.raises(ValueError, match="no point clouds"):
        M.generation_metrics([good], [])
    with pytest.raises(ValueError):
        M.generation_metrics([torch.zeros((5, 2))], [good])          # xyz needed
    with pytest.raises(ValueError):
        M.generation_metrics([good], torch.zeros((2, 5, 2)))


def test_subsample_is_deterministic_without_replacement_and_keeps_short_clouds():
    cloud = torch.arange(5000 * 4, dtype=torch.float32).view(5000, 4)          # row i starts with 4 i: rows are recognisable
    a, b = M.subsample(cloud, 2048, 7), M.subsample(cloud, 2048, 7)
    assert a.shape == (2048, 4) and torch.equal(a, b)
    rows = (a[:, 0] / 4).long()
    assert len(set(rows.tolist())) == 2048 and torch.equal(a, cloud[rows])     # distinct rows of the cloud, whole rows
    assert rows.tolist() == sorted(rows.tolist())                              # in their original order
    assert not torch.equal(M.subsample(cloud, 2048, 8), a)                     # the seed matters
    short = cloud[:100]
    assert torch.equal(M.subsample(short, 2048, 3), short) and torch.equal(M.subsample(short, 100, 3), short)
    with pytest.raises(ValueError):
        M.subsample(cloud, 0, 1)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _brute_nn(q, t):
    """min over t of ((dx*dx + dy*dy) + dz*dz) in fp32, numpy element-wise ops (one rounding each, no FMA)."""
    q = np.ascontiguousarray(q[:, :3], np.float32)
    t = np.ascontiguousarray(t[:, :3], np.float32)
    out = np.empty(len(q), np.float32)
    step = max(1, (1 << 22) // max(1, len(t)))
    for i in range(0, len(q), step):
        qq = q[i:i + step]
        dx = qq[:, None, 0] - t[None, :, 0]
        dy = qq[:, None, 1] - t[None, :, 1]
        dz = qq[:, None, 2] - t[None, :, 2]
        out[i:i + step] = ((dx * dx + dy * dy) + dz * dz).min(1)
    return out


def _ref_cd(xs, ys=None):
    """Chamfer matrix in numpy: brute-force minima, math.fsum, one division per direction"""
    sym = ys is None
    ys = xs if sym else ys
    cd = np.zeros((len(xs), len(ys)))
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            if sym and j <= i:
                continue
            cd[i, j] = (math.fsum(_brute_nn(x, y).astype(np.float64).tolist()) / len(x)
                        + math.fsum(_brute_nn(y, x).astype(np.float64).tolist()) / len(y))
    return cd + cd.T if sym else cd


def synthetic_scene(rng, n):
    """A cloud with a shape of its own: an anisotropic Gaussian blob around a random centre plus a ground ring."""
    centre = rng.uniform(-10.0, 10.0, 3) * np.array([1.0, 1.0, 0.1])
    axes = rng.uniform(2.0, 20.0, 3) * np.array([1.0, 1.0, 0.1])
    blob = rng.standard_normal((n - n // 4, 3)) * axes + centre
    az = rng.uniform(-np.pi, np.pi, n // 4)
    rad = rng.uniform(5.0, 40.0)
    ring = np.stack([rad * np.cos(az), rad * np.sin(az), np.full(n // 4, -1.7)], 1)
    return np.concatenate([blob, ring]).astype(np.float32)


def _two_smallest_gap(m, skip_diag=False):
    """per row: (second smallest - smallest) / smallest"""
    m = np.array(m, np.float64)
    if skip_diag:
        np.fill_diagonal(m, np.inf)
    s = np.sort(m, 1)
    return (s[:, 1] - s[:, 0]) / s[:, 0]


def _dev(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


@pytest.mark.gpu
def test_hand_made_case_on_the_device():
    mats = [torch.tensor(m, dtype=torch.float64, device="cuda") for m in (HAND_GG, HAND_GR, HAND_RR)]
    assert M.set_metrics(*mats) == HAND_ANSWER


@pytest.mark.gpu
def test_generation_metrics_match_the_numpy_restatement():
    n_pts, seed = 512, 2024
    rng = np.random.default_rng(seed)
    gen = [synthetic_scene(rng, n_pts) for _ in range(24)]
    ref = [synthetic_scene(rng, n_pts) for _ in range(24)]
    gg, gr, rr = _ref_cd(gen), _ref_cd(gen, ref), _ref_cd(ref)
    # discrete results are comparable only where no argmin is decided inside the rounding bound: every row that an argmin is
    # taken of has its two smallest entries further apart than 100 x the bound (n * 2^-52 relative, n = 512 points)
    bound = n_pts * 2.0 ** -52
    union = np.block([[gg, gr], [gr.T, rr]])
    gaps = np.concatenate([_two_smallest_gap(gr), _two_smallest_gap(union, skip_diag=True)])
    print("smallest relative gap between a row's two smallest entries:", float(gaps.min()), "bound:", bound)
    assert gaps.min() > 100 * bound
    want = _np_set_metrics(gg, gr, rr)
    assert M.set_metrics_host(gg, gr, rr) == want
    got = M.generation_metrics(_dev(gen), _dev(ref))
    print("device:", got, "numpy:", want)
    for key in ("cov_cd", "nna_cd", "nna_cd_gen", "nna_cd_ref", "n_gen", "n_ref"):
        assert got[key] == want[key], key
    # MMD: a correctly rounded mean of 24 entries, each the sum of two directions that are within (n + 2) * 2^-53 of their
    # reference: (n + 6) * 2^-53 in all, inside the same n * 2^-52
    assert abs(got["mmd_cd"] - want["mmd_cd"]) <= bound * want["mmd_cd"]
    assert isinstance(got["mmd_cd"], float) and isinstance(got["n_gen"], int)
    # the device matrices themselves, entry by entry
    for dev_m, ref_m in ((M.chamfer_matrix(_dev(gen)), gg), (M.chamfer_matrix(_dev(gen), _dev(ref)), gr)):
        assert np.all(np.abs(dev_m.cpu().numpy() - ref_m) <= bound * ref_m)


@pytest.mark.gpu
def test_planted_sets_have_their_known_answers():
    rng = np.random.default_rng(99)
    ref = _dev([synthetic_scene(rng, 512) for _ in range(24)])
    same = M.generation_metrics([c.clone() for c in ref], ref)
    assert same["mmd_cd"] == 0.0 and same["cov_cd"] == 1.0
    # every cloud's nearest OTHER cloud is its copy in the other set, at distance 0: all of them are wrong
    assert same["nna_cd"] == 0.0
    collapsed = M.generation_metrics([ref[5].clone() for _ in range(24)], ref)
    assert collapsed["cov_cd"] == 1 / 24 and collapsed["n_gen"] == 24 and collapsed["n_ref"] == 24
    # the copies of one cloud are each other's nearest neighbours (distance 0, lowest index): all generated right
    assert collapsed["nna_cd_gen"] == 1.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_evaluate(nproc, args, timeout):
    env = dict(os.environ, RLDM_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    launcher = ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
                 "127.0.0.1", "--master-port", str(_free_port())] if nproc > 1 else [sys.executable])
    r = subprocess.run(launcher + ["-m", "rangeldm_amd.evaluate"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 prints ONE JSON object
    return lines[0]


@pytest.mark.gpu
def test_evaluate_generation_one_process_and_two_ranks(tmp_path):
    from rangeldm_amd import evaluate as E
    rng = np.random.default_rng(4)
    gdir, rdir = tmp_path / "gen", tmp_path / "ref"
    gdir.mkdir()
    rdir.mkdir()
    for d, count in ((gdir, 7), (rdir, 6)):
        for i in range(count):
            pts = synthetic_scene(rng, int(rng.integers(900, 3000)))
            np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1).tofile(str(d / f"{i:04d}.bin"))
    out = tmp_path / "one.json"
    args = ["generation", str(gdir), str(rdir), "--points", "512", "--limit", "6", "--seed", "3", "--max-depth", "60"]
    one = _run_evaluate(1, args + ["--json", str(out)], timeout=300)
    res = json.loads(one)
    assert set(res) == {"task", "points", "mmd_cd", "cov_cd", "nna_cd", "nna_cd_gen", "nna_cd_ref", "n_gen", "n_ref", "jsd", "mmd"}
    assert res["task"] == "generation" and res["points"] == 512 and res["n_gen"] == 6 and res["n_ref"] == 6
    assert out.read_text() == one + "\n"
    assert 0.0 < res["mmd_cd"] and 0.0 < res["cov_cd"] <= 1.0 and 0.0 <= res["nna_cd"] <= 1.0 and 0.0 <= res["jsd"] <= 1.0
    # the same clouds through the library, in this process
    files = lambda d: sorted(str(p) for p in d.iterdir() if p.suffix == ".bin")[:6]
    gen = E.load_generation_clouds(files(gdir), 4, 512, 3, 60.0, "cuda")
    ref = E.load_generation_clouds(files(rdir), 4, 512, 3, 60.0, "cuda")
    assert all(c.shape == (512, 3) for c in gen + ref)
    direct = M.generation_metrics(gen, ref)
    assert all(res[k] == direct[k] for k in direct)
    # (only now, after the first launch succeeded) two ranks on this one GPU: byte-identical output
    two = _run_evaluate(2, args, timeout=300)
    assert two == one
