"""Frechet distance over dumped activations, host side (rangeldm_amd.metrics: frechet_distance_host, frd_indices,
load_activations, the argument checks of frechet_distance / gram_f64 / singular_values, the status mapping; `evaluate frd`).

The fixtures under tests/golden/ hold data only.  frechet_cases.npz: per case two activation matrices (stored as fp32; the
fp64 values the reference was given are exactly these) and the value the reference's calculate_frechet_distance returned
for np.mean / np.cov of them (scipy.linalg.sqrtm on the d x d product).  frd_indices_seed0.npy: get_fid's draw,
`random.seed(0); random.sample(range(2097152), 4096)`.

Tolerance against the reference values.  Differences are taken relative to Tr C1 + Tr C2, the scale of the terms the
distance is a difference of (the distance itself is about 0 for identical sets).  Measured, frechet_distance_host against
the fixture values:

    n12_9_40    (rank-deficient product)   1.59e-08
    n40_33_16   (full rank)                2.2e-16
    n64_64_64                              3.6e-15
    same_7_7_5  (identical sets)           5.6e-16

The reference side is sqrtm of a singular product there, so the first figure is sqrtm's noise, not the identity's (the same
formula agrees with it to 1e-15 where the product has full rank).  REF_RTOL is 8 x the worst of them.
"""
import os

import numpy as np
import pytest
import torch

from rangeldm_amd import _lib
from rangeldm_amd import metrics as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_WORST = 1.59e-8              # measured (see above)
REF_RTOL = 8 * REF_WORST         # relative to Tr C1 + Tr C2


def frechet_cases():
    """[(name, x fp64 (n1, d), y fp64 (n2, d), reference value)] from the fixture, in a fixed order."""
    z = np.load(os.path.join(GOLDEN, "frechet_cases.npz"))
    names = sorted(k[:-4] for k in z.files if k.endswith("_ref"))
    return [(n, z[n + "_x"].astype(np.float64), z[n + "_y"].astype(np.float64), float(z[n + "_ref"])) for n in names]


def trace_scale(x, y):
    """Tr C1 + Tr C2 of two activation sets, fp64."""
    a, b = x - x.mean(0), y - y.mean(0)
    return float((a * a).sum() / (len(x) - 1) + (b * b).sum() / (len(y) - 1))


def jacobi_host(m, max_sweeps=60):
    """The scheme of frechet.hip's singular values restated in numpy, a step's pairs at once: one-sided Jacobi on the
    orientation with fewer columns, round-robin pairs over the column count padded to even, a pair skipped when
    |gamma| <= tol sqrt(alpha) sqrt(beta) (tol = sqrt(column length) 2^-52) or a norm is 0, one sweep after the last
    rotation.  Returns (singular values descending, sweeps run).  Only the order inside a reduction differs from the device."""
    m = np.asarray(m, dtype=np.float64)
    w = (m if m.shape[1] <= m.shape[0] else m.T).copy()
    length, c = w.shape
    cpad = c + (c & 1)
    mod = cpad - 1
    tol = np.sqrt(length) * 2.0 ** -52
    b = np.arange(cpad // 2)
    for sweep in range(1, max_sweeps + 1):
        rotations = 0
        for step in range(cpad - 1):
            p = np.where(b == 0, mod, (step + b) % mod)
            q = np.where(b == 0, step, (step + mod - b) % mod)
            p, q = np.minimum(p, q), np.maximum(p, q)
            p, q = p[q < c], q[q < c]
            ap, aq = w[:, p], w[:, q]
            alpha, beta, gamma = (ap * ap).sum(0), (aq * aq).sum(0), (ap * aq).sum(0)
            with np.errstate(all="ignore"):
                rotate = (alpha != 0) & (beta != 0) & ~(np.abs(gamma) <= tol * (np.sqrt(alpha) * np.sqrt(beta)))
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            cs = np.where(rotate, 1.0 / np.sqrt(1.0 + t * t), 1.0)
            sn = np.where(rotate, cs * t, 0.0)
            w[:, p], w[:, q] = cs * ap - sn * aq, sn * ap + cs * aq
            rotations += int(rotate.sum())
        if rotations == 0:
            return np.sort(np.sqrt((w * w).sum(0)))[::-1], sweep
    raise OverflowError(f"still rotating after {max_sweeps} sweeps")


def frechet_restated(x, y):
    """frechet_distance_host with jacobi_host in the place of np.linalg.svd: the device's arithmetic up to reduction order."""
    mu1, mu2 = x.mean(0), y.mean(0)
    a, b = x - mu1, y - mu2
    sv, _ = jacobi_host(a @ b.T)
    diff = mu1 - mu2
    return float(diff.dot(diff) + (a * a).sum() / (len(x) - 1) + (b * b).sum() / (len(y) - 1)
                 - 2.0 * sv.sum() / np.sqrt((len(x) - 1.0) * (len(y) - 1.0)))


def _hadamard16():
    h = np.array([[1.0]])
    for _ in range(4):
        h = np.block([[h, h], [h, -h]])
    return h


def sv_cases():
    """The matrices the singular values are checked on (here through jacobi_host, in tests/test_frechet_gpu.py on the device)."""
    rng = np.random.default_rng(11)
    zero_col = rng.normal(size=(12, 6))
    zero_col[:, 2] = 0.0
    equal_cols = rng.normal(size=(15, 6))
    equal_cols[:, 4] = equal_cols[:, 1]
    rank5 = rng.normal(size=(40, 5)) @ rng.normal(size=(5, 40))
    return [("random_33x20", rng.normal(size=(33, 20))), ("random_20x33", rng.normal(size=(20, 33))),
            ("odd_columns_31x7", rng.normal(size=(31, 7))), ("zero_column", zero_col), ("equal_columns", equal_cols),
            ("rank5_in_40x40", rank5), ("orthogonal", _hadamard16() * np.arange(1.0, 17.0)),
            ("one_by_one", np.array([[-3.5]])), ("random_300x257", rng.normal(size=(300, 257)))]


def property_inputs():
    """(x (150, 40), y (90, 40), v (40,)) of the property comparisons: A B^T is 150 x 90 of rank <= 40; |v|^2 is about Tr C."""
    rng = np.random.default_rng(21)
    x, y = rng.normal(size=(150, 40)), rng.normal(0.2, 1.5, size=(90, 40))
    return x, y, rng.normal(size=40)


def frechet_comparisons(distance):
    """[(name, value of `distance`, value it is compared with, Tr C1 + Tr C2)]: every comparison the tolerance of the distance
    is taken over -- the fixture cases and the rank-deficient pair against frechet_distance_host, swapped arguments against
    each other, identical sets against 0, a shifted copy against |v|^2."""
    out = [(name, distance(x, y), M.frechet_distance_host(x, y), trace_scale(x, y)) for name, x, y, _ in frechet_cases()]
    x, y, v = property_inputs()
    xy = distance(x, y)
    out.append(("rank 40 in 150 x 90", xy, M.frechet_distance_host(x, y), trace_scale(x, y)))
    out.append(("swapped", distance(y, x), xy, trace_scale(x, y)))
    out.append(("identical sets", distance(x, x.copy()), 0.0, trace_scale(x, x)))
    out.append(("shifted copy", distance(x, x + v), float(v.dot(v)), trace_scale(x, x + v)))
    return out


# worst differences of the numpy restatement (jacobi_host / frechet_restated), in units of 2^-52 x the scale: reproduced by
# test_constants_of_the_numpy_restatement below
SV_C_RESTATED = 132.9            # |sigma - np.linalg.svd| / sigma_max over sv_cases(): random_300x257, 12 sweeps
FRD_C_RESTATED = 97.6            # |distance - compared value| / (Tr C1 + Tr C2) over frechet_comparisons(): identical sets


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the HIP library fails the test."""
    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "require_gpu", touched)


def test_fixture_holds_the_cases_the_metric_is_pinned_on():
    cases = frechet_cases()
    assert [(c[0], c[1].shape, c[2].shape) for c in cases] == [
        ("n12_9_40", (12, 40), (9, 40)), ("n40_33_16", (40, 16), (33, 16)), ("n64_64_64", (64, 64), (64, 64)),
        ("same_7_7_5", (7, 5), (7, 5))]
    assert np.array_equal(cases[3][1], cases[3][2])
    assert all(np.isfinite(c[3]) for c in cases)


def test_frd_indices_are_the_reference_draw():
    want = np.load(os.path.join(GOLDEN, "frd_indices_seed0.npy"))
    got = M.frd_indices()
    assert len(got) == 4096 and len(set(got)) == 4096 and np.array_equal(np.asarray(got), want)
    assert M.frd_indices(2097152, 4096, 0) == got
    assert M.frd_indices(seed=1) != got
    small = M.frd_indices(total=50, count=7)
    assert len(small) == 7 and all(0 <= i < 50 for i in small)


@pytest.mark.parametrize("case", frechet_cases(), ids=lambda c: c[0])
def test_host_formula_against_the_reference_values(case):
    name, x, y, ref = case
    got = M.frechet_distance_host(x, y)
    rel = abs(got - ref) / trace_scale(x, y)
    print(f"{name}: host {got!r} reference {ref!r} difference / (Tr C1 + Tr C2) = {rel:.3e}")
    assert rel <= REF_RTOL


def test_host_formula_properties():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(30, 12))
    v = rng.normal(size=12)
    scale = trace_scale(x, x)
    assert abs(M.frechet_distance_host(x, x)) <= 1e-13 * scale
    assert abs(M.frechet_distance_host(x, x + v) - v.dot(v)) <= 1e-13 * (scale + v.dot(v))      # equal covariances
    y = rng.normal(size=(21, 12))
    assert abs(M.frechet_distance_host(x, y) - M.frechet_distance_host(y, x)) <= 1e-13 * trace_scale(x, y)
    for bad in ((x[:1], y), (x, y[:, :5]), (x[0], y)):
        with pytest.raises(ValueError):
            M.frechet_distance_host(*bad)


def test_the_jacobi_scheme_restated_in_numpy_converges_to_the_singular_values():
    rng = np.random.default_rng(3)
    rank3 = rng.normal(size=(24, 3)) @ rng.normal(size=(3, 17))
    for name, m in (("30x13", rng.normal(size=(30, 13))), ("13x30", rng.normal(size=(13, 30))), ("rank 3 in 24x17", rank3),
                    ("1x1", np.array([[-2.0]])), ("orthogonal", np.diag([3.0, 1.0, 2.0, 5.0]))):
        sv, sweeps = jacobi_host(m)
        want = np.linalg.svd(m, compute_uv=False)
        c = np.abs(sv - want).max() / (2.0 ** -52 * want[0])
        print(f"{name}: {sweeps} sweeps, worst difference {c:.2f} x 2^-52 sigma_max")
        # every column takes sweeps * (columns - 1) rotations of a few roundings each, and so does LAPACK's bidiagonalisation
        assert c <= 4 * sweeps * max(1, min(m.shape) - 1) and sweeps < 30
        assert sweeps == 1 or name not in ("1x1", "orthogonal")


def test_constants_of_the_numpy_restatement():
    worst_sv = 0.0
    for name, m in sv_cases():
        sv, sweeps = jacobi_host(m)
        want = np.linalg.svd(m, compute_uv=False)
        c = float(np.abs(sv - want).max() / (2.0 ** -52 * want[0]))
        print(f"{name}: {sweeps} sweeps, worst difference {c:.1f} x 2^-52 sigma_max")
        worst_sv = max(worst_sv, c)
    worst_frd = 0.0
    for name, got, want, scale in frechet_comparisons(frechet_restated):
        c = abs(got - want) / (2.0 ** -52 * scale)
        print(f"{name}: difference {c:.1f} x 2^-52 (Tr C1 + Tr C2)")
        worst_frd = max(worst_frd, c)
    print(f"worst: singular values {worst_sv:.1f}, distance {worst_frd:.1f}")
    # the recorded constants are these worst cases where they were taken; another host's BLAS and summation order move them
    # by a few per cent (94 to 98 seen for the distance), so: inside the factor 8 a tolerance adds, and not inflated
    assert worst_sv <= 8 * SV_C_RESTATED and SV_C_RESTATED <= 2 * worst_sv
    assert worst_frd <= 8 * FRD_C_RESTATED and FRD_C_RESTATED <= 2 * worst_frd


def test_argument_errors_come_before_the_library(no_library):
    x, y = torch.zeros(6, 4), torch.zeros(5, 4)
    with pytest.raises(ValueError, match="at least 2 samples"):
        M.frechet_distance(x[:1], y)
    with pytest.raises(ValueError, match="at least 2 samples"):
        M.frechet_distance(x, y[:1])
    with pytest.raises(ValueError, match="values per sample"):
        M.frechet_distance(x, torch.zeros(5, 3))
    for bad in (torch.zeros(6), torch.zeros(2, 3, 4), torch.zeros(0, 4)):
        with pytest.raises(ValueError, match="2-D"):
            M.frechet_distance(bad, y)
        with pytest.raises(ValueError, match="2-D"):
            M.frechet_distance(x, bad)
    with pytest.raises(ValueError, match="floating-point"):
        M.frechet_distance(x.to(torch.int32), y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.frechet_distance(x, y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.frechet_distance(x.double(), y.half())
    # the two building blocks
    with pytest.raises(ValueError, match="values per row"):
        M.gram_f64(x, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="2-D"):
        M.gram_f64(torch.zeros(6), y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.gram_f64(x, y)
    with pytest.raises(ValueError, match="2-D"):
        M.singular_values(torch.zeros(3))
    with pytest.raises(ValueError, match="max_sweeps"):
        M.singular_values(x, max_sweeps=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.singular_values(x)


def test_status_mapping():
    M._frechet_status(0, "", "call")
    assert issubclass(M.FrechetConvergenceError, RuntimeError)
    with pytest.raises(M.FrechetConvergenceError, match="call: still rotating"):
        M._frechet_status(_lib.RLDM_FRECHET_SWEEP_CAP, "still rotating", "call")
    with pytest.raises(ValueError, match="NaN or inf"):
        M._frechet_status(_lib.RLDM_FRECHET_NONFINITE, "the input holds NaN or inf", "call")
    with pytest.raises(RuntimeError, match="call failed: other") as e:
        M._frechet_status(1, "other", "call")
    assert not isinstance(e.value, M.FrechetConvergenceError)
    assert _lib.RLDM_FRECHET_SWEEP_CAP != _lib.RLDM_FRECHET_NONFINITE and 1 not in (_lib.RLDM_FRECHET_SWEEP_CAP,
                                                                                   _lib.RLDM_FRECHET_NONFINITE)
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "rangeldm_hip.h")).read()
    for name in ("RLDM_FRECHET_SWEEP_CAP", "RLDM_FRECHET_NONFINITE", "RLDM_FRECHET_MAX_SWEEPS"):
        assert f"#define {name} {getattr(_lib, name)} " in header


def test_load_activations(tmp_path):
    rng = np.random.default_rng(1)
    total, count = 4 * 6 * 5, 9
    idx = M.frd_indices(total=total, count=count)
    arrays = {}
    for name in ("b.npy", "a.npy", "c.npy"):             # written out of order: they are read sorted by name
        arrays[name] = rng.normal(size=(4, 6, 5)).astype(np.float32)
        np.save(str(tmp_path / name), arrays[name])
    (tmp_path / "notes.txt").write_text("not an activation file")
    got = M.load_activations(str(tmp_path), idx, total=total, device="cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, count)
    want = np.stack([arrays[n].reshape(-1)[idx] for n in ("a.npy", "b.npy", "c.npy")])
    assert np.array_equal(got.numpy(), want)
    two = M.load_activations(str(tmp_path), idx, limit=2, total=total, device="cpu")
    assert np.array_equal(two.numpy(), want[:2])
    assert "sorted" in M.load_activations.__doc__.lower() and "glob order" in M.load_activations.__doc__
    np.save(str(tmp_path / "bb.npy"), np.zeros(total - 1, np.float32))
    with pytest.raises(ValueError, match=r"bb\.npy.*119 values, expected 120"):
        M.load_activations(str(tmp_path), idx, total=total, device="cpu")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        M.load_activations(str(empty), idx, total=total, device="cpu")


def test_evaluate_frd_argument_parsing():
    from rangeldm_amd import evaluate as E
    a = E.build_parser().parse_args(["frd", "A", "B"])
    assert (a.cmd, a.folder1, a.folder2, a.limit, a.total, a.count, a.json) == ("frd", "A", "B", 1100, 2097152, 4096, None)
    a = E.build_parser().parse_args(["frd", "A", "B", "--limit", "8", "--total", "64", "--count", "16", "--json", "o.json"])
    assert (a.limit, a.total, a.count, a.json) == (8, 64, 16, "o.json")
    E.check_frd_args(a)
    assert E.COMMANDS["frd"] is E.cmd_frd
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["frd", "A"])
    for bad in (["--limit", "1"], ["--total", "8", "--count", "9"], ["--count", "0"]):
        with pytest.raises(ValueError):
            E.check_frd_args(E.build_parser().parse_args(["frd", "A", "B"] + bad))
