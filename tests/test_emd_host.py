"""Earth Mover's Distance, host side: `auction_host`, the sequential numpy restatement of the epsilon-scaling auction of
rangeldm_amd/csrc/emd.hip (the reference tests/test_emd_gpu.py compares the kernel with, bit for bit), validated here
against scipy.optimize.linear_sum_assignment through the certificate the auction returns; and the host-side parts of the
feature: set_metrics_host(name=), the `generation --emd` argument checks, the size errors raised before the device, the
mapping of the kernel's bid-cap status.

The certificate.  With c the fp32 cost matrix, a the returned assignment and p the returned prices, evaluated in fp64:

    slack = max_i [ max_j (-c[i][j] - p[j]) - (-c[i][a(i)] - p[a(i)]) ]                       (>= 0)

LP duality: for ANY permutation b, sum_i c[i][a(i)] <= sum_i c[i][b(i)] + N slack (add the N inequalities
c[i][a(i)] + p[a(i)] <= c[i][b(i)] + p[b(i)] + slack; the prices cancel because a and b are both permutations).  So
0 <= emd - opt <= slack, whatever produced a and p.

The bound on slack.  u = 2^-24 (fp32 unit roundoff), M = max c + max p (final prices: prices only ever rise).  When bidder i
made the bid that won it a(i) = j1 (in the LAST phase: assignments are reset per phase, so every final assignment was made
with the final eps), it computed w[j] = fl(c[i][j] + p[j]), each within u M of the true sum.  Then
    c[i][j1] + p[j1] <= w1 + u M                                             (1 rounding)
    p' = fl(fl(p[j1] + fl(w2 - w1)) + eps) <= p[j1] + (w2 - w1) + eps + 3 u M  (3 roundings, each operand below M)
    hence  c[i][j1] + p' <= w2 + eps + 4 u M
    the true second-best value min_{j != j1} (c[i][j] + p[j]) >= w2 - u M      (1 rounding)
so right after the bid i's slack is at most eps + 5 u M; until i is displaced p[j1] stays and every other price can only
rise, which does not increase the slack.  5 u M = 2.5 * 2^-23 M; the test allows SLACK_ROUNDINGS = 3 * 2^-23 M (the half
covers the second-order (1 + u) factors and the fp64 evaluation), tighter than a guessed 8.
"""
import argparse
import math
import os
from collections import deque

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -7
BID_CAP = 1024                   # bids per point at which a pair is given up
SLACK_ROUNDINGS = 3.0            # in units of 2^-23 (max c + max p): derived above
F = np.float32
EMD_INSTANCES = (1, 2, 4, 8, 16, 24, 32)     # objects per lane of emd_auction_kernel<K>: emd.hip's EMD_LAUNCH(K), held below


# ---- the restatement ------------------------------------------------------------------------------------------------------
def cost_matrix(x, y):
    """c[i][j] = sqrt((dx*dx + dy*dy) + dz*dz) in fp32, one rounding per operation (numpy does not contract)."""
    x = np.ascontiguousarray(np.asarray(x)[:, :3], F)
    y = np.ascontiguousarray(np.asarray(y)[:, :3], F)
    dx = x[:, None, 0] - y[None, :, 0]
    dy = x[:, None, 1] - y[None, :, 1]
    dz = x[:, None, 2] - y[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def first_eps(x, y):
    """0.25f * the largest fp32 side (hi - lo) of the joint bounding box of the two clouds."""
    both = np.concatenate([np.asarray(x)[:, :3], np.asarray(y)[:, :3]]).astype(F)
    return F(0.25) * (both.max(0) - both.min(0)).max()


def auction_host(x, y, eps):
    """The auction of emd.hip, one bid after the other.  Returns (assignment int32 [N], prices fp32 [N], bids, emd), or
    raises OverflowError when bidders still wait after BID_CAP * N bids."""
    c = cost_matrix(x, y)
    n = c.shape[0]
    assert c.shape == (n, n)
    eps = F(eps)
    p = np.zeros(n, F)
    bids, cap = 0, BID_CAP * n
    e = first_eps(x, y)
    while True:
        ek = e if e > eps else eps
        owner = np.full(n, -1, np.int64)
        assign = np.full(n, -1, np.int32)
        fifo = deque(range(n))
        while fifo:
            if bids >= cap:
                raise OverflowError(f"{bids} bids")
            i = fifo.popleft()
            v = -(c[i] + p)
            j1 = int(np.argmax(v))                       # the first maximum: the lowest j
            v1 = v[j1]
            if n > 1:
                v[j1] = -np.inf
                v2 = v.max()
            else:
                v2 = v1
            p[j1] = (p[j1] + (v1 - v2)) + ek
            bids += 1
            prev = owner[j1]
            owner[j1] = i
            assign[i] = j1
            if prev >= 0:
                assign[prev] = -1
                fifo.append(int(prev))
        if not e > eps:
            break
        e = e * F(0.25)
    return assign, p, bids, fixed_order_mean(c[np.arange(n), assign])


def fixed_order_mean(values):
    """fp64 sum, ascending index, one add after the other; divided once."""
    s = 0.0
    for v in np.asarray(values, np.float64).tolist():
        s += v
    return s / len(values)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def lidar_like(rng, n):
    """A spinning-sensor sweep: ranges 3 .. 70 m (ground-heavy), 64 beams between -25 and +3 degrees, any azimuth."""
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.choice(np.linspace(-25.0, 3.0, 64), n))
    r = np.minimum(3.0 + rng.exponential(12.0, n), 70.0)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F)


def instance_sizes():
    """For every instance K: its first size 64 K_prev + 1 (nearly half the lanes' last slot is a pad; 3 for K = 1), 64 K - 1
    (one pad) and 64 K (none: the ring starts full)."""
    sizes, prev = [], None
    for k in EMD_INSTANCES:
        sizes += [3 if prev is None else 64 * prev + 1, 64 * k - 1, 64 * k]
        prev = k
    return sizes


def emd_cases():
    """[(name, x, y)]: the inputs the restatement and the kernel are both checked on."""
    rng = np.random.default_rng(20240917)
    first = (1, 2, 777, 2048)
    cases = [(f"lidar_{n}", lidar_like(rng, n), lidar_like(rng, n)) for n in first]
    base = lidar_like(rng, 500)
    cases.append(("permutation_of_itself", base, base[rng.permutation(500)]))
    cases.append(("grid_8", rng.integers(-8, 9, (600, 3)).astype(F), rng.integers(-8, 9, (600, 3)).astype(F)))
    cases.append(("grid_2", rng.integers(-2, 3, (400, 3)).astype(F), rng.integers(-2, 3, (400, 3)).astype(F)))
    cases.append(("all_identical", np.full((300, 3), 1.5, F), np.full((300, 3), 1.5, F)))
    blob = lambda cx, n: (rng.standard_normal((n, 3)) * 0.05 + np.array([cx, 0.0, 0.0])).astype(F)
    # two tight clusters 60 m apart, 200 + 56 points on one side and 56 + 200 on the other: 144 points must cross
    cases.append(("two_clusters", np.concatenate([blob(0.0, 200), blob(60.0, 56)]),
                  np.concatenate([blob(0.0, 56), blob(60.0, 200)])))
    # every instance of the kernel at its first size, one short of full and full (a generator of their own: the cases above
    # stay what they were); then ties on the instances K = 2 and K = 24 and on full rings
    rng = np.random.default_rng(20250720)
    cases += [(f"lidar_{n}", lidar_like(rng, n), lidar_like(rng, n)) for n in instance_sizes() if n not in first]
    grid = lambda r, n: rng.integers(-r, r + 1, (n, 3)).astype(F)
    cases += [(f"grid_2_{n}", grid(2, n), grid(2, n)) for n in (100, 128, 1100, 1536)]
    cases += [(f"grid_8_{n}", grid(8, n), grid(8, n)) for n in (64, 1100)]
    cases += [(f"all_identical_{n}", np.full((n, 3), 1.5, F), np.full((n, 3), 1.5, F)) for n in (64, 128, 1536)]
    return cases


def check_certificate(name, x, y, assign, prices, bids, emd, eps=EPS):
    """The assertions of the module docstring, on any (assignment, prices, bids, emd) claimed for the pair (x, y)."""
    from scipy.optimize import linear_sum_assignment
    n = len(x)
    assign, prices = np.asarray(assign), np.asarray(prices)
    assert sorted(assign.tolist()) == list(range(n)), f"{name}: not a permutation"
    c = cost_matrix(x, y).astype(np.float64)
    rows, cols = linear_sum_assignment(c)
    opt = c[rows, cols].sum() / n
    value = -c - prices.astype(np.float64)[None, :]
    slack = float((value.max(1) - value[np.arange(n), assign]).max())
    big = float(c.max() + prices.max())
    bound = eps + SLACK_ROUNDINGS * 2.0 ** -23 * big
    rounding = 4 * n * 2.0 ** -53 * float(c.max()) + 1e-300       # two fp64 sums of n terms below max c, each divided once
    print(f"{name}: n {n} emd {emd:.9g} opt {opt:.9g} emd-opt {emd - opt:.3e} slack {slack:.6e} slack-eps {slack - eps:.3e} "
          f"bound-eps {bound - eps:.3e} max c+p {big:.4g} bids/point {bids / n:.2f}")
    assert emd == fixed_order_mean(c[np.arange(n), assign]), f"{name}: the value is not the mean of its assignment"
    assert -rounding <= emd - opt <= slack + rounding, name
    assert 0.0 <= slack <= bound, name
    assert bids <= BID_CAP * n / 8, name
    return slack


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", emd_cases(), ids=lambda c: c[0])
def test_auction_host_is_certified_against_linear_sum_assignment(case):
    name, x, y = case
    assign, prices, bids, emd = auction_host(x, y, EPS)
    assert assign.dtype == np.int32 and prices.dtype == np.float32
    check_certificate(name, x, y, assign, prices, bids, emd)


def test_the_instances_are_the_ones_emd_hip_launches():
    # the sizes of emd_cases() follow EMD_INSTANCES; an instance added to or taken from emd.hip fails here until it follows
    import re
    text = open(os.path.join(ROOT, "rangeldm_amd", "csrc", "emd.hip")).read()
    launched = tuple(int(k) for k in re.findall(r"EMD_LAUNCH\((\d+)\)", text))
    assert launched == EMD_INSTANCES and EMD_INSTANCES[-1] * 64 == M.EMD_MAX_POINTS
    assert instance_sizes() == [3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537,
                                2047, 2048]
    sizes = {len(x) for _, x, _ in emd_cases()}
    assert set(instance_sizes()) <= sizes and {100, 1100} <= sizes
    assert len({name for name, _, _ in emd_cases()}) == len(emd_cases())


def test_auction_host_known_answers():
    # one point: the distance itself, one bid per phase
    a, p, bids, emd = auction_host(np.array([[0, 0, 0]], F), np.array([[3, 4, 0]], F), EPS)
    assert a.tolist() == [0] and emd == 5.0
    # a permutation of a well-separated cloud is matched back exactly: EMD 0
    grid = np.stack(np.meshgrid(*[np.arange(4.0)] * 3), -1).reshape(-1, 3).astype(F)
    perm = np.random.default_rng(1).permutation(len(grid))
    a, _, _, emd = auction_host(grid, grid[perm], EPS)
    assert emd == 0.0 and np.array_equal(perm[a], np.arange(len(grid)))
    # the schedule: ext = 160 -> e_0 = 40, and it is the caller's eps, exactly, that runs the last phase
    assert first_eps(np.array([[-80, 0, 0]], F), np.array([[80, 1, 1]], F)) == F(40.0)
    # the cap is a condition: with an absurdly small eps on duplicate-heavy input the restatement gives up, it does not return
    tiny = np.zeros((3, 3), F)
    with pytest.raises(OverflowError):
        auction_host(np.concatenate([tiny, tiny + 1]), np.concatenate([tiny + 0.5, tiny + 0.5]), 1e-12)


def test_set_metrics_host_names_its_keys():
    gg, gr, rr = [[0, 1, 9], [1, 0, 9], [9, 9, 0]], [[1, 2, 5], [3, 1, 4], [2, 6, 2]], [[0, 7, 1], [7, 0, 8], [1, 8, 0]]
    cd = M.set_metrics_host(gg, gr, rr)
    assert cd == M.set_metrics_host(gg, gr, rr, name="cd")
    assert set(cd) == {"mmd_cd", "cov_cd", "nna_cd", "nna_cd_gen", "nna_cd_ref", "n_gen", "n_ref"}
    emd = M.set_metrics_host(gg, gr, rr, name="emd")
    assert emd == {"mmd_emd": 4 / 3, "cov_emd": 2 / 3, "nna_emd": 0.5, "nna_emd_gen": 2 / 3, "nna_emd_ref": 1 / 3,
                   "n_gen": 3, "n_ref": 3}
    assert [emd[k.replace("_cd", "_emd")] for k in cd] == list(cd.values())


def test_size_errors_come_before_the_device():
    a, b = torch.zeros((5, 3)), torch.zeros((6, 3))
    with pytest.raises(ValueError, match="one-to-one matching"):
        M.emd_matrix([a, b])
    with pytest.raises(ValueError, match="one-to-one matching"):
        M.emd_matrix([a], [b])
    with pytest.raises(ValueError, match="one-to-one matching"):
        M.emd_pairs([a, a], [a, b])
    with pytest.raises(ValueError, match="one-to-one matching.*2048|2048.*one-to-one"):
        M.emd_matrix([torch.zeros((2049, 3))])
    with pytest.raises(ValueError, match="one-to-one matching"):
        M.generation_metrics([a], [b], emd=True)
    with pytest.raises(ValueError, match="empty"):
        M.emd_matrix([a, torch.zeros((0, 3))])
    with pytest.raises(ValueError, match="eps"):
        M.emd_matrix([a, a], eps=0.0)
    with pytest.raises(ValueError):
        M.emd_pairs([a], [a, a])


def test_bid_cap_status_is_an_error_that_names_the_pair():
    from rangeldm_amd import _lib
    assert M._emd_status(0, "") is None
    with pytest.raises(M.EmdBidCapError, match=r"pair \(3, 5\) reached the bid cap"):
        M._emd_status(_lib.RLDM_EMD_BID_CAP, "pair (3, 5) reached the bid cap of 1024 x 2048 bids; no value is returned")
    assert issubclass(M.EmdBidCapError, RuntimeError)
    with pytest.raises(RuntimeError, match="bad shape") as info:
        M._emd_status(1, "bad shape")
    assert not isinstance(info.value, M.EmdBidCapError)


def test_generation_emd_arguments(tmp_path):
    from rangeldm_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["generation", "g", "r"])
    assert a.emd is False and a.emd_eps == 2.0 ** -7
    a = ap.parse_args(["generation", "g", "r", "--emd", "--emd-eps", "0.03125", "--points", "1024"])
    assert a.emd is True and a.emd_eps == 0.03125
    E.check_emd_args(a)
    with pytest.raises(ValueError, match="2048"):
        E.check_emd_args(argparse.Namespace(points=4096, emd_eps=EPS))
    with pytest.raises(ValueError, match="emd-eps"):
        E.check_emd_args(argparse.Namespace(points=2048, emd_eps=0.0))
    # a cloud that is left with fewer than --points points: the file is named
    files = [str(tmp_path / "0000.bin"), str(tmp_path / "0001.bin")]
    E.require_emd_sizes(files, [torch.zeros((512, 3)), torch.zeros((512, 3))], 512)
    with pytest.raises(ValueError, match=r"0001\.bin: 400 points"):
        E.require_emd_sizes(files, [torch.zeros((512, 3)), torch.zeros((400, 3))], 512)
    # `python -m rangeldm_amd.evaluate chamfer` and friends do not grow the flag
    with pytest.raises(SystemExit):
        ap.parse_args(["chamfer", "a", "b", "--emd"])
