"""Counter-based normals: the device generator of the samplers and trainers, and its numpy statement.

One function defines every normal this module ever produces,

    normal(seed, stream, row, sample, e)        seed uint64; stream, row, sample uint32; 0 <= e < 2^31

* Block.  Philox4x32-10 (Salmon et al., Random123) with key (seed & 0xffffffff, seed >> 32) and counter (e >> 2, sample, row, stream).
* Normals.  The block's words (o0, o1, o2, o3) give four normals by two Box-Muller pairs, (o0, o1) -> (z0, z1), (o2, o3) -> (z2, z3);
  element e takes z[e & 3].  ln, sin and cos are written out in fp32 + - * / sqrt, one rounding each (normals_from_bits_host), and
  csrc/rng.hip evaluates the same sequence: the device equals this file bit for bit.
* Streams.  stream = 4 * draw + purpose; a *draw* is one call that consumes noise.  Purpose 0: x_T and any plain randn (row 0);
  1: the step noise of row r; 2: the known-region noise of row r; 3: the re-noise of row r.
* Samples.  sample = sample_offset + b, b the position in the call's batch: the noise of a sample does not depend on the batch
  size, on how the sampler cuts a batch into lanes, or on which rank draws it.

A generator is (seed, draw).  Every consuming call uses the current draw and advances it by one; `at()` addresses a given
(draw, purpose, row) without consuming."""
import ctypes as C

import numpy as np

PURPOSE_PLAIN, PURPOSE_STEP, PURPOSE_KNOWN, PURPOSE_RENOISE = 0, 1, 2, 3
MAX_DRAW = 1 << 30          # stream = 4 * draw + purpose is 32 bits
MAX_PER_SAMPLE = 1 << 31    # the element index of a sample is 31 bits
MAX_SAMPLES = 1 << 32       # the sample index is 32 bits

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def _check_address(seed, draw, purpose, row):
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed {seed} is not a uint64")
    if not 0 <= int(draw) < MAX_DRAW:
        raise ValueError(f"draw {draw} outside [0, 2^30)")
    if int(purpose) not in (0, 1, 2, 3):
        raise ValueError(f"purpose {purpose} outside 0..3")
    if not 0 <= int(row) < 1 << 32:
        raise ValueError(f"row {row} is not a uint32")


def _check_shape(B, per_sample, sample_offset):
    if B < 0 or per_sample < 0:
        raise ValueError("negative shape")
    if per_sample >= MAX_PER_SAMPLE:
        raise ValueError(f"per_sample {per_sample} >= 2^31")
    if sample_offset < 0 or sample_offset + B > MAX_SAMPLES:
        raise ValueError(f"sample_offset {sample_offset} + B {B} > 2^32")


class DeviceGenerator:
    """(seed, draw): the state of the counter-based generator.  Nothing lives on the device."""

    def __init__(self, seed=0):
        self.manual_seed(seed)

    def manual_seed(self, seed):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} is not a uint64")
        self._seed, self._draw = seed, 0
        return self

    @property
    def seed(self):
        return self._seed

    @property
    def draw(self):
        return self._draw

    def get_state(self):
        return (self._seed, self._draw)

    def set_state(self, state):
        seed, draw = (int(v) for v in state)
        _check_address(seed, draw, 0, 0)
        self._seed, self._draw = seed, draw
        return self

    def next_draw(self):
        """The current draw, consumed: the generator moves to the next one."""
        if self._draw >= MAX_DRAW:
            raise ValueError("the generator has consumed all 2^30 draws of its seed: manual_seed another one")
        d = self._draw
        self._draw += 1
        return d

    def at(self, draw=None, purpose=0, row=0):
        """An address (seed, draw, purpose, row) of this generator's streams; consumes nothing.  `randn(shape, at)` draws there."""
        draw = self._draw if draw is None else int(draw)
        _check_address(self._seed, draw, purpose, row)
        return StreamAddress(self._seed, draw, int(purpose), int(row))


class StreamAddress:
    """A fixed (seed, draw, purpose, row): what `DeviceGenerator.at` returns and `randn` accepts in place of a generator."""

    def __init__(self, seed, draw, purpose=0, row=0):
        _check_address(seed, draw, purpose, row)
        self.seed, self.draw, self.purpose, self.row = int(seed), int(draw), int(purpose), int(row)

    @property
    def stream(self):
        return 4 * self.draw + self.purpose


# ---- the numpy statement ------------------------------------------------------------------------------------------------------
def philox_host(counters, key):
    """Philox4x32-10: counters uint32 [n, 4], key (k0, k1) -> uint32 [n, 4]."""
    c = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4).astype(np.uint64)
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _SH) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


_F = np.float32
_LN_C = [_F(1.0 / 11.0), _F(1.0 / 9.0), _F(1.0 / 7.0), _F(1.0 / 5.0), _F(1.0 / 3.0), _F(1.0)]
_SIN_C = [_F(1.0 / 362880.0), _F(-1.0 / 5040.0), _F(1.0 / 120.0), _F(-1.0 / 6.0), _F(1.0)]
_COS_C = [_F(-1.0 / 3628800.0), _F(1.0 / 40320.0), _F(-1.0 / 720.0), _F(1.0 / 24.0), _F(-0.5), _F(1.0)]
_LN2_HI, _LN2_LO, _SQRT_HALF, _HALF_PI = _F(0.693359375), _F(-2.12194440e-4), _F(0.70710678), _F(1.5707963267948966)


def uniforms_from_bits(x, y):
    """u1 = (float(x >> 9) + 0.5) * 2^-23 in [2^-24, 1 - 2^-24], u2 = float(y >> 8) * 2^-24 in [0, 1): both exact in fp32."""
    x, y = np.asarray(x, dtype=np.uint32), np.asarray(y, dtype=np.uint32)
    u1 = ((x >> np.uint32(9)).astype(_F) + _F(0.5)) * _F(2.0 ** -23)
    u2 = (y >> np.uint32(8)).astype(_F) * _F(2.0 ** -24)
    return u1, u2


def _horner(coef, v):
    q = np.full_like(v, coef[0])
    for c in coef[1:]:
        q = q * v + c           # two roundings: numpy has no fused multiply-add
    return q


def _box_muller(x, y):
    """(x, y) uint32 -> (r cos(2 pi u2), r sin(2 pi u2)), every line one fp32 operation per element (csrc/rng.hip: box_muller)."""
    u1, u2 = uniforms_from_bits(x, y)
    ub = u1.view(np.uint32)
    e = (ub >> np.uint32(23)).astype(np.int32) - 126
    m = ((ub & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(_F)
    low = m < _SQRT_HALF
    m = np.where(low, m + m, m)
    e = np.where(low, e - 1, e)
    s = (m - _F(1.0)) / (m + _F(1.0))
    s2 = s * s
    lnm = (s + s) * _horner(_LN_C, s2)
    ef = e.astype(_F)
    ln = ef * _LN2_HI + (ef * _LN2_LO + lnm)
    r = np.sqrt(_F(-2.0) * ln)
    t = _F(4.0) * u2
    kf = np.rint(t)
    a = (t - kf) * _HALF_PI
    a2 = a * a
    sn = a * _horner(_SIN_C, a2)
    cs = _horner(_COS_C, a2)
    k = kf.astype(np.int32) & 3
    odd = (k & 1) == 1
    c = np.where(odd, sn, cs)
    d = np.where(odd, cs, sn)
    c = np.where((k == 1) | (k == 2), -c, c)
    d = np.where((k == 2) | (k == 3), -d, d)
    return r * c, r * d


def normals_from_bits_host(bits):
    """uint32 [n, 4] Philox words -> fp32 [n, 4] normals."""
    b = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1, 4)
    z0, z1 = _box_muller(b[:, 0], b[:, 1])
    z2, z3 = _box_muller(b[:, 2], b[:, 3])
    return np.stack([z0, z1, z2, z3], axis=1).astype(_F)


def block_counters(B, per_sample, stream, row, sample_offset):
    """The counters (e >> 2, sample, row, stream) of a [B, per_sample] draw: uint32 [B * ceil(per_sample / 4), 4]."""
    nblk = (per_sample + 3) // 4
    c = np.empty((B, nblk, 4), dtype=np.uint32)
    c[:, :, 0] = np.arange(nblk, dtype=np.uint32)[None, :]
    c[:, :, 1] = ((np.arange(B, dtype=np.uint64) + np.uint64(sample_offset)) & _MASK).astype(np.uint32)[:, None]
    c[:, :, 2] = np.uint32(row)
    c[:, :, 3] = np.uint32(stream)
    return c.reshape(-1, 4)


def randn_host(shape, seed, draw=0, purpose=0, row=0, sample_offset=0):
    """fp32 numpy array of `shape` (shape[0] the sample axis): normal(seed, 4 * draw + purpose, row, sample_offset + b, e)."""
    shape = tuple(int(v) for v in shape)
    B, per = (shape[0], int(np.prod(shape[1:], dtype=np.int64))) if shape else (1, 1)
    _check_address(seed, draw, purpose, row)
    _check_shape(B, per, int(sample_offset))
    if B * per == 0:
        return np.zeros(shape, dtype=_F)
    key = (int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    bits = philox_host(block_counters(B, per, 4 * int(draw) + int(purpose), row, int(sample_offset)), key)
    z = normals_from_bits_host(bits).reshape(B, -1)[:, :per]
    return np.ascontiguousarray(z).reshape(shape)


def timesteps_host(B, seed, draw, num_train_timesteps, sample_offset=0):
    """B training timesteps in [0, T): t_b = (o0 * T) >> 32 with o0 the first word of the Philox block at counter
    (0, sample_offset + b, 0, 4 * draw + 1), key from `seed` -- the step-noise stream's row 0, which a trainer never uses for noise
    (its noise is the plain stream, purpose 0).  int64 numpy array."""
    _check_address(seed, draw, PURPOSE_STEP, 0)
    _check_shape(B, 1, int(sample_offset))
    key = (int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    bits = philox_host(block_counters(B, 1, 4 * int(draw) + PURPOSE_STEP, 0, int(sample_offset)), key)
    return ((bits[:, 0].astype(np.uint64) * np.uint64(num_train_timesteps)) >> _SH).astype(np.int64)


# ---- the device -----------------------------------------------------------------------------------------------------------------
def _resolve(generator):
    """an address as it is; None for a generator, whose current draw the caller consumes"""
    if isinstance(generator, StreamAddress):
        return generator
    if isinstance(generator, DeviceGenerator):
        return None
    raise TypeError(f"randn needs a DeviceGenerator or an address from DeviceGenerator.at, not {type(generator).__name__}")


def randn(shape, generator, sample_offset=0, device="cuda", purpose=0, row=0, out=None):
    """fp32 device tensor of `shape` drawn by csrc/rng.hip; shape[0] is the sample axis.  With a DeviceGenerator it consumes one
    draw (stream 4 * draw + purpose, row `row`); with an address from `DeviceGenerator.at` it draws there and consumes nothing."""
    import torch
    from . import _lib
    shape = tuple(int(v) for v in shape)
    if not shape:
        raise ValueError("randn needs at least the sample axis")
    B, per = shape[0], int(np.prod(shape[1:], dtype=np.int64))
    addr = _resolve(generator)
    if addr is None:
        _check_address(generator.seed, min(generator.draw, MAX_DRAW - 1), purpose, row)
        _check_shape(B, per, int(sample_offset))
        addr = StreamAddress(generator.seed, generator.next_draw(), purpose, row)
    else:
        _check_shape(B, per, int(sample_offset))
    if out is None:
        out = torch.empty(shape, device=device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous fp32 device tensor of `shape`")
    if B * per:
        _lib.check(_lib.lib().rldm_randn(C.c_void_p(out.data_ptr()), B, per, addr.seed, addr.stream, addr.row, int(sample_offset),
                                         _lib.stream_ptr(out.device)), "rldm_randn")
    return out


def randn_rows(rows, shape, generator, draw, purpose, sample_offset=0, device="cuda"):
    """[rows, *shape]: row r is randn(shape, generator.at(draw, purpose, r)) -- the tensor an explicit step_noise= / known_noise= /
    renoise_noise= argument carries for the rows a sampler draws by itself.  Consumes nothing."""
    import torch
    zs = torch.empty((int(rows), *shape), device=device, dtype=torch.float32)
    for r in range(int(rows)):
        randn(shape, generator.at(draw, purpose, r), sample_offset, device, out=zs[r])
    return zs
