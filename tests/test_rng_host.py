"""CPU: the numpy statement of the counter-based generator (rangeldm_amd/rng.py) -- Philox4x32-10 on its known answers, the accuracy of
the written-out fp32 ln / sin / cos against the same formulas in fp64, the distribution of a fixed stream, the independence of a
sample's noise from how a batch is cut, and the generator's state and refusals.  tests/test_rng_gpu.py holds the device to this
statement bit for bit."""
import numpy as np
import pytest
import torch

from rangeldm_amd import rng

N = 4_194_304
KEY = (0x1234, 0x5678)


@pytest.fixture(scope="module")
def stream():
    """N normals of key (0x1234, 0x5678), counters (q, 0, 0, 0): the words, the normals, computed once."""
    c = np.zeros((N // 4, 4), dtype=np.uint32)
    c[:, 0] = np.arange(N // 4, dtype=np.uint32)
    bits = rng.philox_host(c, KEY)
    return bits, rng.normals_from_bits_host(bits)


def test_philox_known_answers():
    zero = rng.philox_host(np.zeros((1, 4), dtype=np.uint32), (0, 0))[0]
    ones = rng.philox_host(np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(v) for v in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_uniforms_are_exact_and_inside_their_ranges():
    x = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32)
    u1, u2 = rng.uniforms_from_bits(x, x)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert [float(v) for v in u1] == [2.0 ** -24, 2.0 ** -24, 1.5 * 2.0 ** -23, 1.0 - 2.0 ** -24]
    assert [float(v) for v in u2] == [0.0, 2.0 ** -24, 2.0 ** -23, 1.0 - 2.0 ** -24]


def test_transform_accuracy_against_fp64(stream):
    """randn_host's fp32 ln / sin / cos against the same Box-Muller in fp64 on the same (u1, u2), over 4 194 304 normals with key
    (0x1234, 0x5678).  Measured: 5.992e-07 absolute, 2.486e-07 relative to max(1, |z|).  The gates are twice that: 1.1984e-06 and
    4.972e-07."""
    bits, z = stream
    ref = []
    for x, y in ((bits[:, 0], bits[:, 1]), (bits[:, 2], bits[:, 3])):
        u1, u2 = (v.astype(np.float64) for v in rng.uniforms_from_bits(x, y))
        r = np.sqrt(-2.0 * np.log(u1))
        ref += [r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)]
    ref = np.stack(ref, axis=1)
    err = np.abs(z.astype(np.float64) - ref)
    e_abs, e_rel = float(err.max()), float((err / np.maximum(1.0, np.abs(ref))).max())
    print(f"transform vs fp64: abs {e_abs:.4e}, rel {e_rel:.4e}")
    assert np.isfinite(z).all() and float(np.abs(z).max()) <= 5.77
    assert e_abs <= 1.1984e-06 and e_rel <= 4.972e-07


def test_distribution_of_a_fixed_stream(stream):
    """z-scores of mean, variance, skewness and excess kurtosis, and sqrt(N) D of Kolmogorov-Smirnov against Phi, of the fixed
    stream above (a fixed computation, not a sample of a test statistic): measured -0.21, -0.28, +0.16, +1.18 and 0.71.
    Gates: |z| <= 4 and sqrt(N) D <= 1.95."""
    z = stream[1].reshape(-1).astype(np.float64)
    n = z.size
    m, v = z.mean(), z.var()
    d = z - m
    scores = dict(mean=m * np.sqrt(n), variance=(v - 1.0) / np.sqrt(2.0 / n), skewness=(d ** 3).mean() / v ** 1.5 / np.sqrt(6.0 / n),
                  kurtosis=((d ** 4).mean() / v ** 2 - 3.0) / np.sqrt(24.0 / n))
    cdf = torch.special.ndtr(torch.from_numpy(np.sort(z))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = np.sqrt(n) * max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    print({k: round(float(s), 3) for k, s in scores.items()}, f"sqrt(N) D = {ks:.3f}")
    for k, s in scores.items():
        assert abs(s) <= 4.0, (k, s)
    assert ks <= 1.95


def test_a_sample_does_not_depend_on_how_the_batch_is_cut():
    shape = (3, 7, 5)                                           # 105 elements: the last block of a sample is cut
    whole = rng.randn_host((5, *shape), seed=9, draw=3, purpose=1, row=6)
    parts = np.concatenate([rng.randn_host((2, *shape), 9, 3, 1, 6, sample_offset=0), rng.randn_host((3, *shape), 9, 3, 1, 6, sample_offset=2)])
    assert whole.dtype == np.float32 and whole.tobytes() == parts.tobytes()
    single = rng.randn_host((1, *shape), 9, 3, 1, 6, sample_offset=4)
    assert single.tobytes() == whole[4:].tobytes()


def test_every_word_of_the_address_changes_the_values():
    base = dict(seed=5, draw=2, purpose=1, row=3, sample_offset=4)
    z = rng.randn_host((2, 33), **base)
    for k, v in (("draw", 3), ("purpose", 2), ("row", 4), ("sample_offset", 5), ("seed", 6), ("seed", 5 + (1 << 32))):
        other = rng.randn_host((2, 33), **dict(base, **{k: v}))
        assert not np.array_equal(z, other), k
        assert np.abs(z - other).max() > 0.5, k                 # (another stream, not a perturbation)
    # sample_offset + 1 shifts the samples: sample 1 of the first is sample 0 of the second
    assert np.array_equal(z[1], rng.randn_host((2, 33), **dict(base, sample_offset=5))[0])


def test_generator_state_round_trip_and_draw_counting():
    g = rng.DeviceGenerator(seed=(1 << 63) + 5)
    assert (g.seed, g.draw) == ((1 << 63) + 5, 0)
    assert g.next_draw() == 0 and g.next_draw() == 1 and g.draw == 2
    a = g.at(purpose=3, row=7)
    assert (a.seed, a.draw, a.purpose, a.row, a.stream) == (g.seed, 2, 3, 7, 11) and g.draw == 2       # at() consumes nothing
    st = g.get_state()
    g.next_draw()
    h = rng.DeviceGenerator().set_state(st)
    assert h.get_state() == st and h.next_draw() == 2
    assert g.manual_seed(8).get_state() == (8, 0)
    last = rng.DeviceGenerator(1).set_state((1, rng.MAX_DRAW - 1))
    assert last.next_draw() == rng.MAX_DRAW - 1
    with pytest.raises(ValueError, match="2\\^30"):
        last.next_draw()


def test_timesteps_host_is_the_scaled_first_word():
    t = rng.timesteps_host(6, seed=3, draw=2, num_train_timesteps=1000, sample_offset=10)
    c = np.array([[0, 10 + b, 0, 4 * 2 + 1] for b in range(6)], dtype=np.uint32)
    want = [(int(w) * 1000) >> 32 for w in rng.philox_host(c, (3, 0))[:, 0]]
    assert t.dtype == np.int64 and t.tolist() == want and all(0 <= v < 1000 for v in want)
    assert rng.timesteps_host(2, 3, 2, 1000, sample_offset=12).tolist() == want[2:4]


def test_refusals():
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="uint64"):
            rng.DeviceGenerator(bad)
        with pytest.raises(ValueError, match="uint64"):
            rng.randn_host((1, 4), seed=bad)
    g = rng.DeviceGenerator(1)
    with pytest.raises(ValueError, match="draw"):
        g.set_state((1, rng.MAX_DRAW))
    with pytest.raises(ValueError, match="draw"):
        g.at(draw=rng.MAX_DRAW)
    with pytest.raises(ValueError, match="draw"):
        rng.randn_host((1, 4), 1, draw=rng.MAX_DRAW)
    with pytest.raises(ValueError, match="purpose"):
        g.at(purpose=4)
    with pytest.raises(ValueError, match="row"):
        g.at(row=1 << 32)
    with pytest.raises(ValueError, match="2\\^31"):
        rng.randn_host((1, 1 << 31), 1)
    with pytest.raises(ValueError, match="2\\^32"):
        rng.randn_host((3, 4), 1, sample_offset=(1 << 32) - 2)
    assert rng.randn_host((3, 4), 1, sample_offset=(1 << 32) - 3).shape == (3, 4)
    # the device entry refuses the same before it touches the device, and a refused call consumes no draw
    for shape, kw in (((1, 1 << 31), {}), ((3, 4), dict(sample_offset=(1 << 32) - 2)), ((2, 4), dict(purpose=5)), ((), {})):
        with pytest.raises(ValueError):
            rng.randn(shape, g, **kw)
    assert g.draw == 0
    with pytest.raises(TypeError, match="DeviceGenerator"):
        rng.randn((1, 4), torch.Generator())
