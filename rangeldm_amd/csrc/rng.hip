// rng.hip -- counter-based normals on gfx950: the noise of every sampler, trainer and plain randn, drawn on the device.
//
//   normal(seed, stream, row, sample, e)      seed uint64; stream, row, sample uint32; 0 <= e < 2^31
//
// is a pure function, restated in numpy (rangeldm_amd/rng.py: philox_host, normals_from_bits_host, randn_host); the device
// equals the restatement bit for bit (tests/test_rng_gpu.py).  Nothing here depends on the batch size, on how a batch is cut
// into lanes or ranks, or on the grid: a thread computes whole Philox blocks from their counters.
//
// Block.     Philox4x32-10 (Salmon et al., Random123): key (seed & 0xffffffff, seed >> 32), counter (e >> 2, sample, row, stream);
//            multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.  Known answers: include/rangeldm_hip.h.
// Normals.   The words (o0, o1, o2, o3) give z0, z1 from (o0, o1) and z2, z3 from (o2, o3) by Box-Muller; element e is z[e & 3].
//            A pair (x, y):  u1 = (float(x >> 9) + 0.5) * 2^-23 in [2^-24, 1 - 2^-24],  u2 = float(y >> 8) * 2^-24 in [0, 1), both
//            exact;  r = sqrt(-2 ln u1),  z_even = r cos(2 pi u2),  z_odd = r sin(2 pi u2).  No NaN, no inf, |z| <= 5.77.
// Arithmetic. ln, sin and cos are written out in fp32 + - * / sqrt, one rounding per operation (eval_common.h's f_mul .. f_sqrt, the
//            pragma below, -ffp-contract=off in the Makefile), in the order rng.py's normals_from_bits_host states:
//   ln u1     u1 = m * 2^e, m in [0.5, 1) by bit operations; if m < fp32(0.70710678) then m = 2 m, e = e - 1;
//             s = (m - 1) / (m + 1), s2 = s s, p = Horner in s2 over 1/11, 1/9, 1/7, 1/5, 1/3, 1;  ln m = (s + s) p;
//             ln u1 = e * 0.693359375 + (e * -2.12194440e-4 + ln m)
//   sin, cos  t = 4 u2 (exact), k = rint(t), f = t - k in [-1/2, 1/2] (exact), a = f * fp32(pi / 2), a2 = a a;
//             sin a = a * Horner in a2 over 1/9!, -1/7!, 1/5!, -1/3!, 1;  cos a = Horner in a2 over -1/10!, 1/8!, -1/6!, 1/4!, -1/2!, 1;
//             (cos, sin)(2 pi u2) = (c, s), (-s, c), (-c, -s), (s, -c) for k & 3 = 0, 1, 2, 3
//            No intermediate is subnormal (|s| >= 2^-25 or 0, |a| >= 2^-22 or 0, r >= 2^-11.5), so the flush mode does not matter.
//
//   rng_fill_kernel     a thread per Philox block of a sample ([B][per_sample]: a block never straddles two samples; grid.y walks
//                       the samples, grid.x the blocks of one); a 16-byte store where the block is whole and its address aligned,
//                       scalar stores otherwise (the tail of a sample whose size is no multiple of 4, and every block of the
//                       samples such a size leaves unaligned).  No workgroup waits on another; nothing is read but the sampler's
//                       16-byte record and step word.  Measured: 2.7 TB/s written on 134 M normals, bound by
//                       the arithmetic of the correctly rounded division and square root, not by HBM.
#include "eval_common.h"
#include "kernels.h"
#include "../../include/rangeldm_hip.h"

#include <cstdint>
#include <string>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) every operation below is rounded once

namespace {

struct Block4 { uint32_t v[4]; };
struct Normal4 { float v[4]; };

__device__ __forceinline__ Block4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Block4{{c0, c1, c2, c3}};
}

// (x, y) -> (r cos(2 pi u2), r sin(2 pi u2)): the sequence of the header, operation by operation
__device__ __forceinline__ void box_muller(uint32_t x, uint32_t y, float& z_even, float& z_odd) {
    const float u1 = f_mul(f_add((float)(x >> 9), 0.5f), 1.1920928955078125e-07f);     // 2^-23
    const float u2 = f_mul((float)(y >> 8), 5.9604644775390625e-08f);                  // 2^-24
    // ln u1
    const uint32_t ub = __float_as_uint(u1);
    int e = (int)(ub >> 23) - 126;
    float m = __uint_as_float((ub & 0x007fffffu) | 0x3f000000u);
    if (m < 0.70710678f) {
        m = f_add(m, m);
        e -= 1;
    }
    const float s = f_div(f_sub(m, 1.0f), f_add(m, 1.0f));
    const float s2 = f_mul(s, s);
    float p = (float)(1.0 / 11.0);                            // 1/11
    p = f_add(f_mul(p, s2), (float)(1.0 / 9.0));              // 1/9
    p = f_add(f_mul(p, s2), (float)(1.0 / 7.0));              // 1/7
    p = f_add(f_mul(p, s2), (float)(1.0 / 5.0));              // 1/5
    p = f_add(f_mul(p, s2), (float)(1.0 / 3.0));              // 1/3
    p = f_add(f_mul(p, s2), 1.0f);
    const float lnm = f_mul(f_add(s, s), p);
    const float ef = (float)e;
    const float ln = f_add(f_mul(ef, 0.693359375f), f_add(f_mul(ef, -2.12194440e-4f), lnm));
    const float r = f_sqrt(f_mul(-2.0f, ln));
    // sin, cos of 2 pi u2
    const float t = f_mul(4.0f, u2);
    const float kf = rintf(t);
    const float a = f_mul(f_sub(t, kf), (float)1.5707963267948966);
    const float a2 = f_mul(a, a);
    float qs = (float)(1.0 / 362880.0);                       // 1/9!
    qs = f_add(f_mul(qs, a2), (float)(-1.0 / 5040.0));        // -1/7!
    qs = f_add(f_mul(qs, a2), (float)(1.0 / 120.0));          // 1/5!
    qs = f_add(f_mul(qs, a2), (float)(-1.0 / 6.0));           // -1/3!
    qs = f_add(f_mul(qs, a2), 1.0f);
    const float sn = f_mul(a, qs);
    float qc = (float)(-1.0 / 3628800.0);                     // -1/10!
    qc = f_add(f_mul(qc, a2), (float)(1.0 / 40320.0));        // 1/8!
    qc = f_add(f_mul(qc, a2), (float)(-1.0 / 720.0));         // -1/6!
    qc = f_add(f_mul(qc, a2), (float)(1.0 / 24.0));           // 1/4!
    qc = f_add(f_mul(qc, a2), -0.5f);
    qc = f_add(f_mul(qc, a2), 1.0f);
    const int k = (int)kf & 3;
    const float c = (k & 1) ? sn : qc, d = (k & 1) ? qc : sn;
    const float cs = (k == 1 || k == 2) ? -c : c;   // cos: c, -s, -c, s
    const float ss = (k == 2 || k == 3) ? -d : d;   // sin: s, c, -s, -c
    z_even = f_mul(r, cs);
    z_odd = f_mul(r, ss);
}

__device__ __forceinline__ Normal4 normals_from_bits(const Block4& o) {
    Normal4 z;
    box_muller(o.v[0], o.v[1], z.v[0], z.v[1]);
    box_muller(o.v[2], o.v[3], z.v[2], z.v[3]);
    return z;
}

__global__ void __launch_bounds__(256) rng_fill_kernel(const rldm::RngFillParams p) {
    uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32), draw = p.draw, sample0 = p.sample0, row = p.row;
    if (p.record) {
        k0 = p.record[0]; k1 = p.record[1]; draw = p.record[2];
        sample0 += p.record[3];
    }
    if (p.step_ptr) row += (uint32_t)*p.step_ptr;
    const uint32_t stream = 4u * draw + p.purpose;
    // grid.y walks the samples, grid.x the blocks of one sample (per_sample < 2^31: a block index fits 29 bits): no division
    const uint32_t nblk = (uint32_t)((p.per_sample + 3) >> 2);
    for (uint32_t b = blockIdx.y; b < (uint32_t)p.B; b += gridDim.y) {
        float* const base = p.out + (long long)b * p.per_sample;
        for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < nblk; q += gridDim.x * 256u) {
            const Normal4 z = normals_from_bits(philox4x32_10(q, sample0 + b, row, stream, k0, k1));
            const long long e0 = (long long)q << 2;
            float* dst = base + e0;
            if (e0 + 4 <= p.per_sample && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<float4*>(dst) = make_float4(z.v[0], z.v[1], z.v[2], z.v[3]);
            } else {
                for (int j = 0; j < 4 && e0 + j < p.per_sample; ++j) dst[j] = z.v[j];
            }
        }
    }
}

__global__ void rng_record_kernel(uint32_t* rec, uint32_t k0, uint32_t k1, uint32_t draw, uint32_t sample_offset) {
    if (threadIdx.x == 0) { rec[0] = k0; rec[1] = k1; rec[2] = draw; rec[3] = sample_offset; }
}

__global__ void __launch_bounds__(256) rng_philox_kernel(const uint32_t* __restrict__ ctr, uint32_t k0, uint32_t k1, long long n,
                                                         uint32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Block4 o = philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = o.v[j];
}

__global__ void __launch_bounds__(256) rng_normals_kernel(const uint32_t* __restrict__ bits, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Normal4 z = normals_from_bits(Block4{{bits[4 * i], bits[4 * i + 1], bits[4 * i + 2], bits[4 * i + 3]}});
    for (int j = 0; j < 4; ++j) out[4 * i + j] = z.v[j];
}

}  // namespace

namespace rldm {

int launch_rng_fill(const RngFillParams& p, hipStream_t stream) {
    const long long nblk = (p.per_sample + 3) >> 2;
    if (nblk == 0 || p.B <= 0) return 0;
    // about 8192 workgroups at the most: enough to fill the chip several times over, few enough that a thread amortises its set-up
    const unsigned gy = (unsigned)(p.B > 1024 ? 1024 : p.B);
    const long long want = (nblk + 255) / 256, cap = 8192 / gy > 0 ? 8192 / gy : 1;
    const unsigned gx = (unsigned)(want > cap ? cap : want);
    hipLaunchKernelGGL(rng_fill_kernel, dim3(gx, gy), dim3(256), 0, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_rng_record(unsigned* record, unsigned long long seed, unsigned draw, unsigned sample_offset, hipStream_t stream) {
    hipLaunchKernelGGL(rng_record_kernel, dim3(1), dim3(64), 0, stream, record, (uint32_t)seed, (uint32_t)(seed >> 32), draw, sample_offset);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace rldm

extern "C" {

int rldm_randn(float* out, int64_t B, int64_t per_sample, uint64_t seed, uint32_t stream_id, uint32_t row, uint64_t sample_offset,
               void* stream) {
    RLDM_REQUIRE(out, "null argument");
    RLDM_REQUIRE(B >= 0 && B <= 0x7fffffff && per_sample >= 0, "bad shape");
    RLDM_REQUIRE(per_sample < (1LL << 31), "per_sample must be below 2^31 (the element index of a sample is 31 bits)");
    RLDM_REQUIRE(sample_offset + (uint64_t)B <= (1ULL << 32), "sample_offset + B must not exceed 2^32 (the sample index is 32 bits)");
    rldm::RngFillParams p{};
    p.out = out;
    p.per_sample = per_sample;
    p.B = (int)B;
    p.purpose = stream_id & 3u;
    p.draw = stream_id >> 2;
    p.seed = seed;
    p.row = row;
    p.sample0 = (uint32_t)sample_offset;
    return rldm::launch_rng_fill(p, reinterpret_cast<hipStream_t>(stream));
}

int rldm_rng_philox(const uint32_t* counters, const uint32_t key[2], int64_t n, uint32_t* out, void* stream) {
    RLDM_REQUIRE(counters && key && out && n >= 0, "null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(rng_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       counters, key[0], key[1], (long long)n, out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_rng_normals_from_bits(const uint32_t* bits, int64_t n, float* out, void* stream) {
    RLDM_REQUIRE(bits && out && n >= 0, "null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(rng_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       bits, (long long)n, out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
