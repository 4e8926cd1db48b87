"""Earth Mover's Distance on the device (rangeldm_amd/csrc/emd.hip: emd_auction_kernel; rangeldm_amd.metrics.emd_matrix /
emd_pairs / generation_metrics(emd=True); `evaluate generation --emd`).

The kernel is compared BIT FOR BIT -- assignment, prices, bid count, value -- with tests/test_emd_host.py's sequential numpy
restatement `auction_host` on emd_cases() -- every instance K of the kernel at its first size, one short of full and full,
ties on full rings -- and its own output is put through the same certificate against
scipy.optimize.linear_sum_assignment (check_certificate: permutation, 0 <= emd - opt <= slack, slack <= eps + roundings,
bids <= cap / 8), which would hold even if the restatement were wrong.  Then the properties the drivers rely on: an entry
depends on its two clouds and eps alone (strides, symmetric against rectangular, row blocks, two calls, the pair form), the
set metrics on top, and the driver as one process and as two ranks.  No test provokes the bid cap on the device.
"""
import json

import numpy as np
import pytest
import torch

from rangeldm_amd import metrics as M
from test_emd_host import EPS, auction_host, check_certificate, emd_cases, fixed_order_mean, cost_matrix, lidar_like
from test_generation_metrics import _run_evaluate

pytestmark = pytest.mark.gpu


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def _small_set(seed, count, n):
    rng = np.random.default_rng(seed)
    return [lidar_like(rng, n) for _ in range(count)]


@pytest.mark.parametrize("case", emd_cases(), ids=lambda c: c[0])
def test_kernel_equals_auction_host_bit_for_bit_and_is_certified(case):
    name, x, y = case
    emd, asg, price, bids = M.emd_matrix(_dev([x]), _dev([y]), eps=EPS, return_assignment=True)
    assert emd.dtype == torch.float64 and tuple(emd.shape) == (1, 1) and tuple(asg.shape) == (1, 1, len(x))
    emd, asg, price, bids = float(emd[0, 0]), asg[0, 0].cpu().numpy(), price[0, 0].cpu().numpy(), int(bids[0, 0])
    # the certificate first: it does not depend on the restatement
    check_certificate(name + " (device)", x, y, asg, price, bids, emd)
    h_asg, h_price, h_bids, h_emd = auction_host(x, y, EPS)
    print(f"{name}: device bids {bids} host bids {h_bids}; device emd {emd!r} host emd {h_emd!r}; "
          f"assignments differ at {int((asg != h_asg).sum())}, prices at {int((price.view(np.int32) != h_price.view(np.int32)).sum())}")
    assert bids == h_bids
    assert np.array_equal(asg, h_asg)
    assert np.array_equal(price.view(np.int32), h_price.view(np.int32))          # bit patterns
    assert emd == h_emd
    assert emd == fixed_order_mean(cost_matrix(x, y)[np.arange(len(x)), h_asg])


@pytest.mark.parametrize("n", (100, 1100))              # K = 2 and K = 24: the grid-index decoding had only run with K = 4
def test_every_matrix_entry_equals_the_single_pair_call(n):
    xs, ys = _small_set(51 + n, 3, n), _small_set(52 + n, 2, n)
    dx, dy = _dev(xs), _dev(ys)
    pair = lambda a, b: [t[0, 0] for t in M.emd_matrix([a], [b], eps=EPS, return_assignment=True)]
    same = lambda got, want: all(torch.equal(g, w) for g, w in zip(got, want))       # value, assignment, prices, bids
    rect = M.emd_matrix(dx, dy, eps=EPS, return_assignment=True)
    assert tuple(rect[0].shape) == (3, 2) and tuple(rect[1].shape) == (3, 2, n)
    for i in range(3):
        for j in range(2):
            assert same([t[i, j] for t in rect], pair(dx[i], dy[j])), (i, j)
    emd, asg, price, bids = M.emd_matrix(dx, eps=EPS, return_assignment=True)        # the symmetric route
    for i in range(3):
        assert emd[i, i] == 0 and bids[i, i] == 0
        for j in range(i + 1, 3):
            want = pair(dx[i], dx[j])
            assert same([emd[i, j], asg[i, j], price[i, j], bids[i, j]], want), (i, j)
            assert emd[j, i] == want[0] and bids[j, i] == want[3] and emd[i, j] > 0  # the mirror entry
            assert torch.all(asg[j, i] == -1)


def test_strides_3_4_5():
    rng = np.random.default_rng(5)
    xs, ys = _small_set(11, 3, 300), _small_set(12, 2, 300)
    want = M.emd_matrix(_dev(xs), _dev(ys), return_assignment=True)
    pad = lambda c, k: np.concatenate([c, rng.uniform(-1e3, 1e3, (len(c), k - 3)).astype(np.float32)], 1)
    for kx, ky in ((4, 3), (3, 5), (5, 4)):
        got = M.emd_matrix(_dev([pad(c, kx) for c in xs]), _dev([pad(c, ky) for c in ys]), return_assignment=True)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (kx, ky)


def test_symmetric_equals_rectangular_above_the_diagonal():
    xs = _dev(_small_set(21, 5, 200))
    s_emd, s_asg, s_price, s_bids = M.emd_matrix(xs, return_assignment=True)
    r_emd, r_asg, r_price, r_bids = M.emd_matrix(xs, [c.clone() for c in xs], return_assignment=True)
    assert torch.equal(s_emd, s_emd.t()) and torch.equal(s_bids, s_bids.t())
    assert torch.all(torch.diagonal(s_emd) == 0) and torch.all(torch.diagonal(s_bids) == 0)
    for i in range(5):
        for j in range(i + 1, 5):
            assert s_emd[i, j] == r_emd[i, j] and s_bids[i, j] == r_bids[i, j] and s_emd[i, j] > 0
            assert torch.equal(s_asg[i, j], r_asg[i, j]) and torch.equal(s_price[i, j], r_price[i, j])
            assert torch.all(s_asg[j, i] == -1)                          # below the diagonal: not computed, and marked so


def test_row_blocks_two_calls_and_the_pair_form():
    xs, ys = _dev(_small_set(31, 4, 256)), _dev(_small_set(32, 4, 256))
    whole = M.emd_matrix(xs, ys, return_assignment=True)
    again = M.emd_matrix(xs, ys, return_assignment=True)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    for block in (1, 2, 4):
        for lo in range(0, 4, block):
            part = M.emd_matrix(xs[lo:lo + block], ys, return_assignment=True)
            assert all(torch.equal(p, w[lo:lo + block]) for p, w in zip(part, whole)), (block, lo)
    pairs = M.emd_pairs(xs, ys)
    assert pairs.dtype == torch.float64 and torch.equal(pairs, torch.diagonal(whole[0]))
    # another eps is another (certified) answer, not an error
    coarse = M.emd_pairs(xs, ys, eps=0.25)
    # (both lie in [opt, opt + eps + roundings]; 1e-4 is above 3 * 2^-23 (max c + max p) for these clouds, max c + p < 280)
    assert torch.all(coarse >= pairs - (2.0 ** -7 + 1e-4)) and torch.all(coarse <= pairs + (0.25 + 1e-4))


def test_generation_metrics_with_emd_match_the_numpy_statement():
    gen, ref = _small_set(41, 24, 256), _small_set(42, 24, 256)
    dgen, dref = _dev(gen), _dev(ref)
    got = M.generation_metrics(dgen, dref, emd=True)
    plain = M.generation_metrics(dgen, dref)
    assert {k: got[k] for k in plain} == plain                           # the Chamfer half is what it was
    assert set(got) - set(plain) == {"mmd_emd", "cov_emd", "nna_emd", "nna_emd_gen", "nna_emd_ref"}
    gg, gr, rr = M.emd_matrix(dgen).cpu().numpy(), M.emd_matrix(dgen, dref).cpu().numpy(), M.emd_matrix(dref).cpu().numpy()
    want = M.set_metrics_host(gg, gr, rr, name="emd")
    print("device:", {k: got[k] for k in want}, "numpy:", want)
    assert {k: got[k] for k in want} == want
    # the matrices under those reductions are the restatement's: a sample of entries, bit for bit
    for i, j in ((0, 0), (3, 17), (23, 23), (11, 5)):
        assert gr[i, j] == auction_host(gen[i], ref[j], EPS)[3]
    for i, j in ((0, 1), (7, 20)):
        assert gg[i, j] == gg[j, i] == auction_host(gen[i], gen[j], EPS)[3]
        assert rr[i, j] == rr[j, i] == auction_host(ref[i], ref[j], EPS)[3]
    assert 0.0 < got["mmd_emd"] and 0.0 < got["cov_emd"] <= 1.0 and 0.0 <= got["nna_emd"] <= 1.0


def test_evaluate_generation_emd_one_process_and_two_ranks(tmp_path):
    rng = np.random.default_rng(4)
    gdir, rdir = tmp_path / "gen", tmp_path / "ref"
    gdir.mkdir()
    rdir.mkdir()
    for d, count in ((gdir, 6), (rdir, 5)):
        for i in range(count):
            pts = lidar_like(rng, int(rng.integers(900, 3000)))
            np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1).tofile(str(d / f"{i:04d}.bin"))
    args = ["generation", str(gdir), str(rdir), "--points", "256", "--seed", "3"]
    plain = _run_evaluate(1, args, timeout=300)
    one = _run_evaluate(1, args + ["--emd"], timeout=300)
    res = json.loads(one)
    emd_keys = {"mmd_emd", "cov_emd", "nna_emd", "nna_emd_gen", "nna_emd_ref", "emd_eps"}
    assert set(res) - set(json.loads(plain)) == emd_keys and res["emd_eps"] == 2.0 ** -7
    # without --emd: the object the Chamfer-only driver prints, byte for byte
    assert plain == json.dumps({k: v for k, v in res.items() if k not in emd_keys}, sort_keys=True)
    assert set(json.loads(plain)) == {"task", "points", "mmd_cd", "cov_cd", "nna_cd", "nna_cd_gen", "nna_cd_ref", "n_gen", "n_ref",
                                      "jsd", "mmd"}
    assert 0.0 < res["mmd_emd"] and 0.0 < res["cov_emd"] <= 1.0 and 0.0 <= res["nna_emd"] <= 1.0
    # (only now, after the first launches succeeded) two ranks on this one GPU: byte-identical output
    assert _run_evaluate(2, args + ["--emd"], timeout=300) == one
    assert _run_evaluate(2, args, timeout=300) == plain
