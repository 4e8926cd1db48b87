// The PatchGAN discriminator's training kernels (include/rangeldm_hip.h: rldm_train_disc_*; reference: NLayerDiscriminator,
// vae/sgm/modules/autoencoding/lpips/model/model.py:18-89, and GeneralLPIPSWithDiscriminator after disc_start).
//   - 4x4 convolution, zero padding 1 on BOTH axes (W does not wrap here), stride 1 | 2: forward, data gradient (stride 2: the four
//     output parities as four 2x2 convolutions over dy), weight gradient.  bf16 MFMA 32x32x16, fp32 accumulation.
//   - BatchNorm2d in training mode (+ eval-mode forward) fused with LeakyReLU(0.2), forward and backward; fp64 sums in a fixed order.
//   - LeakyReLU(0.2), the hinge loss, the generator term, the adaptive weight + gradient mix.
// Nothing here keeps state or scratch of its own: workspaces are the caller's.  The element-wise arithmetic is restated expression by
// expression on the host (discriminator.batchnorm_host, hinge_d_loss_host): this file is compiled without FMA contraction.
#include "train_common.h"

#include <algorithm>
#include <cstdint>
#include <string>

using namespace rldm::train;

namespace {

// ---- 4x4 convolution: forward and data gradient --------------------------------------------------------------------------------
// One gather kernel.  The produced tensor is [B][Wo][Ho][N], the gathered one [B][Wi][Hi][K]; w = bf16 [N][16][Kpad], tap t = 4 i + j.
//   mode 0  forward:               produced (wo, ho) under tap (i, j) reads (s wo + i - 1, s ho + j - 1)
//   mode 1  data gradient, s = 1:  produced (wi, hi) under tap (i, j) of the flipped copy reads dy (wi + i - 2, hi + j - 2)
//   mode 2  data gradient, s = 2:  grid plane z = (pw, ph) produces the pixels of that parity; only the taps i = pw (mod 2), j = ph
//                                  (mod 2) meet a sample: dy ((wi + i - 2) / 2, (hi + j - 2) / 2), four taps of sixteen
// Outside the gathered tensor is zero on both axes.
struct DcConv {
    const float* x; const bf16_t* w; const float* bias; float* y;
    int B, Wi, Hi, K, Kpad, Wo, Ho, N, mode, stride;
};

// D[channel][pixel]: lane (pixel l & 31, half l >> 5) holds channels (r & 3) + 8 (r >> 2) + 4 half of its pixel (train_conv.hip:
// tr_conv_kernel).  A workgroup owns 32 pixels x 64 channels; its four waves split the TAPS (wave v: taps [v T / 4, (v + 1) T / 4) in
// order, all of K under each) and meet in LDS, where wave 0 adds ((w0 + w1) + w2) + w3: at the discriminator's sizes a launch has a few
// hundred tiles, and a wave that walked all sixteen taps alone (the first form of this kernel: 64 x 128 tiles, one workgroup per CU)
// spent its time waiting for its own loads.  The order is fixed, so the result does not depend on the launch (both modes of
// rldm_train_deterministic).  FAST: K % 16 == 0 (16-byte loads of the gathered rows, no tail).
template <bool FAST>
__global__ __launch_bounds__(256) void dc_conv_kernel(const DcConv p) {
    __shared__ float red[3][32][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, kg = lane >> 5;
    const bool planes = p.mode == 2;
    const int pw = planes ? (int)(blockIdx.z >> 1) : 0, ph = planes ? (int)(blockIdx.z & 1) : 0, step = planes ? 2 : 1;
    const int Wc = planes ? (p.Wo - pw + 1) >> 1 : p.Wo, Hc = planes ? (p.Ho - ph + 1) >> 1 : p.Ho;
    const int P = p.B * Wc * Hc;
    const int px0 = blockIdx.x * 32;
    const int n0 = blockIdx.y * 64;
    if (n0 >= p.N || px0 >= P) return;                               // (uniform over the workgroup: nobody is left at the barrier)
    const int px = px0 + l31;
    const bool pxok = px < P;
    const int pc = pxok ? px : 0;
    const int hc = pc % Hc, t1 = pc / Hc, wc = t1 % Wc, b = t1 / Wc;
    const int wo = wc * step + pw, ho = hc * step + ph;
    const int r0 = n0 + l31, r1 = r0 + 32;                           // this lane's weight rows (A operands)
    const bool ok0 = r0 < p.N, ok1 = r1 < p.N;
    const size_t rstride = (size_t)16 * p.Kpad;
    const bf16_t* w0 = p.w + (size_t)(ok0 ? r0 : 0) * rstride + 8 * kg;
    const bf16_t* w1 = p.w + (size_t)(ok1 ? r1 : 0) * rstride + 8 * kg;
    const bool vec = (p.K & 3) == 0;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const int ntaps = planes ? 4 : 16, tpw = ntaps >> 2;
    for (int tt = wave * tpw; tt < (wave + 1) * tpw; ++tt) {
        const int i = planes ? pw + 2 * (tt >> 1) : tt >> 2, j = planes ? ph + 2 * (tt & 1) : tt & 3;
        int sw, sh;
        if (p.mode == 0) {
            sw = wo * p.stride + i - 1;
            sh = ho * p.stride + j - 1;
        } else {
            sw = wo + i - 2;
            sh = ho + j - 2;
            if (planes) { sw >>= 1; sh >>= 1; }                      // (even by construction; -2 >> 1 = -1 stays outside)
        }
        const bool live = pxok && sw >= 0 && sw < p.Wi && sh >= 0 && sh < p.Hi;
        const float* xrow = p.x + (live ? ((size_t)b * p.Wi + sw) * p.Hi + sh : (size_t)0) * p.K + 8 * kg;
        const size_t toff = (size_t)(4 * i + j) * p.Kpad;
        if (FAST) {
#pragma unroll 4
            for (int c0 = 0; c0 < p.Kpad; c0 += 16) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(w0 + toff + c0), a1 = *reinterpret_cast<const uint4*>(w1 + toff + c0);
                const float4 x0 = *reinterpret_cast<const float4*>(xrow + c0), x1 = *reinterpret_cast<const float4*>(xrow + c0 + 4);
                uint4 u;
                u.x = rldm::pack_bf16x2(x0.x, x0.y); u.y = rldm::pack_bf16x2(x0.z, x0.w);
                u.z = rldm::pack_bf16x2(x1.x, x1.y); u.w = rldm::pack_bf16x2(x1.z, x1.w);
                if (!live) u = make_uint4(0u, 0u, 0u, 0u);
                const bf16x8 bv = __builtin_bit_cast(bf16x8, u);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), bv, acc1, 0, 0, 0);
            }
        } else {
            for (int c0 = 0; c0 < p.Kpad; c0 += 16) {
                uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0;
                if (ok0) a0 = *reinterpret_cast<const uint4*>(w0 + toff + c0);
                if (ok1) a1 = *reinterpret_cast<const uint4*>(w1 + toff + c0);
                const int valid = live ? p.K - (c0 + 8 * kg) : 0;
                float f[8];
                if (vec && valid >= 8) {
                    const float4 q0 = *reinterpret_cast<const float4*>(xrow + c0), q1 = *reinterpret_cast<const float4*>(xrow + c0 + 4);
                    f[0] = q0.x; f[1] = q0.y; f[2] = q0.z; f[3] = q0.w; f[4] = q1.x; f[5] = q1.y; f[6] = q1.z; f[7] = q1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = e < valid ? xrow[c0 + e] : 0.f;
                }
                uint4 u;
                u.x = rldm::pack_bf16x2(f[0], f[1]); u.y = rldm::pack_bf16x2(f[2], f[3]);
                u.z = rldm::pack_bf16x2(f[4], f[5]); u.w = rldm::pack_bf16x2(f[6], f[7]);
                const bf16x8 bv = __builtin_bit_cast(bf16x8, u);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), bv, acc1, 0, 0, 0);
            }
        }
    }
    if (wave) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { red[wave - 1][r][lane] = acc0[r]; red[wave - 1][16 + r][lane] = acc1[r]; }
    }
    __syncthreads();
    if (wave || !pxok) return;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] += red[v][r][lane]; acc1[r] += red[v][16 + r][lane]; }
    float* yrow = p.y + (((size_t)b * p.Wo + wo) * p.Ho + ho) * p.N;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = n0 + 32 * h + (r & 3) + 8 * (r >> 2) + 4 * kg;
            if (ch >= p.N) continue;
            float v = h ? acc1[r] : acc0[r];
            if (p.bias) v += p.bias[ch];
            yrow[ch] = v;
        }
}

// ---- 4x4 convolution: weight gradient -------------------------------------------------------------------------------------------
// dw[n][c][t] = sum over output pixels of dy[px][n] x[src(px, t)][c]: per tap a GEMM with the pixels as K.  Grid (64 x 64 (n, c)
// tiles, 16 taps, K slices); a workgroup stages 32 pixels of dy [64 channels] and of the tap's gathered x [64 channels] as bf16,
// transposed ([channel][pixel], row pitch 80 bytes: an odd number of 16-byte slots) and each wave owns a 32 x 32 quadrant.  The next
// chunk's global loads are in flight while the MFMAs of this one run.  A slice's tile goes to part[slice][N][Cin][16] (or, with one
// slice, is added to dw directly); dc_wgrad_reduce_kernel adds the slices in order.
struct DcWgrad {
    const float* dy; const float* x; float* out;
    int B, Wi, Hi, Cin, Wo, Ho, N, stride, P, cps, direct;
};

__device__ __forceinline__ void dc_load4(const float* __restrict__ row, int c, int C, bool vec, float* v) {
    if (vec && c + 3 < C) {
        const float4 q = *reinterpret_cast<const float4*>(row + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < C ? row[c + e] : 0.f;
    }
}

__global__ __launch_bounds__(256) void dc_wgrad_kernel(const DcWgrad p) {
    constexpr int PITCH = 40;                                        // bf16 per LDS row: 32 pixels + 8
    __shared__ __attribute__((aligned(16))) bf16_t sa[64 * PITCH];
    __shared__ __attribute__((aligned(16))) bf16_t sb[64 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kg = lane >> 5;
    const int ctiles = (p.Cin + 63) / 64;
    const int n0 = ((int)blockIdx.x / ctiles) * 64, c0 = ((int)blockIdx.x % ctiles) * 64;
    const int t = blockIdx.y, ti = t >> 2, tj = t & 3;
    const int nchunks = (p.P + 31) / 32;
    const int chunk0 = blockIdx.z * p.cps, chunk1 = min(chunk0 + p.cps, nchunks);
    const int pp = tid >> 4, cq = tid & 15;                          // staging: pixel pair, channel quad
    const bool vecA = (p.N & 3) == 0, vecB = (p.Cin & 3) == 0;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ra[2][4], rb[2][4];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { ra[q][e] = 0.f; rb[q][e] = 0.f; }
            const int px = chunk * 32 + 2 * pp + q;
            if (px < p.P) {
                const int ho = px % p.Ho, t1 = px / p.Ho, wo = t1 % p.Wo, b = t1 / p.Wo;
                dc_load4(p.dy + (size_t)px * p.N, n0 + 4 * cq, p.N, vecA, ra[q]);
                const int sw = wo * p.stride + ti - 1, sh = ho * p.stride + tj - 1;
                if (sw >= 0 && sw < p.Wi && sh >= 0 && sh < p.Hi)
                    dc_load4(p.x + (((size_t)b * p.Wi + sw) * p.Hi + sh) * p.Cin, c0 + 4 * cq, p.Cin, vecB, rb[q]);
            }
        }
    };
    if (chunk0 < chunk1) fetch(chunk0);
    for (int chunk = chunk0; chunk < chunk1; ++chunk) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *reinterpret_cast<uint32_t*>(sa + (4 * cq + e) * PITCH + 2 * pp) = rldm::pack_bf16x2(ra[0][e], ra[1][e]);
            *reinterpret_cast<uint32_t*>(sb + (4 * cq + e) * PITCH + 2 * pp) = rldm::pack_bf16x2(rb[0][e], rb[1][e]);
        }
        __syncthreads();
        if (chunk + 1 < chunk1) fetch(chunk + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 a = *reinterpret_cast<const uint4*>(sa + (32 * (wave & 1) + l31) * PITCH + 16 * kk + 8 * kg);
            const uint4 bv = *reinterpret_cast<const uint4*>(sb + (32 * (wave >> 1) + l31) * PITCH + 16 * kk + 8 * kg);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
        }
    }
    const int c = c0 + 32 * (wave >> 1) + l31;
    if (c >= p.Cin) return;
    float* out = p.out + (p.direct ? (size_t)0 : (size_t)blockIdx.z * p.N * p.Cin * 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = n0 + 32 * (wave & 1) + (r & 3) + 8 * (r >> 2) + 4 * kg;
        if (n >= p.N) continue;
        const size_t idx = ((size_t)n * p.Cin + c) * 16 + t;
        if (p.direct) out[idx] += acc[r];
        else out[idx] = acc[r];
    }
}

// dw[e] += ((0 + part[0][e]) + part[1][e]) + ...
__global__ __launch_bounds__(256) void dc_wgrad_reduce_kernel(const float* __restrict__ part, int slices, size_t n, float* __restrict__ dw) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float a = 0.f;
    for (int s = 0; s < slices; ++s) a += part[(size_t)s * n + e];
    dw[e] += a;
}

// ---- BatchNorm2d + LeakyReLU(0.2) -----------------------------------------------------------------------------------------------
__device__ __forceinline__ float dc_lrelu(float z) { return z > 0.f ? z : 0.2f * z; }
__device__ __forceinline__ float dc_lrelu_slope(float z) { return z > 0.f ? 1.f : 0.2f; }

// grid (ceil(C / 64), ceil(M / 256)): partial s of channel c = rows [256 s, 256 s + 256); lane k of 4 adds rows s0 + k, s0 + k + 4,
// ... in order, the lanes meet k = 0 .. 3.  part[s][c] = (sum x, sum x^2) or, BWD, (sum dz, sum dz xhat); fp64.
template <bool BWD>
__global__ __launch_bounds__(256) void dc_bn_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ save, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, long long M, int C, double* __restrict__ part) {
    __shared__ double sh[2][4][64];
    const int cl = threadIdx.x & 63, k = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const long long r0 = (long long)blockIdx.y * 256, r1 = r0 + 256 < M ? r0 + 256 : M;
    double a0 = 0.0, a1 = 0.0;
    if (c < C) {
        float mean = 0.f, rstd = 0.f, g = 0.f, bt = 0.f;
        if (BWD) { mean = save[c]; rstd = save[C + c]; g = gamma[c]; bt = beta[c]; }
        for (long long r = r0 + k; r < r1; r += 4) {
            const float v = x[(size_t)r * C + c];
            if (!BWD) {
                a0 += (double)v;
                a1 += (double)v * (double)v;
            } else {
                const float xh = (v - mean) * rstd, z = xh * g + bt, dz = dy[(size_t)r * C + c] * dc_lrelu_slope(z);
                a0 += (double)dz;
                a1 += (double)dz * (double)xh;
            }
        }
    }
    sh[0][k][cl] = a0;
    sh[1][k][cl] = a1;
    __syncthreads();
    if (k == 0 && c < C) {
        double* d = part + ((size_t)blockIdx.y * C + c) * 2;
        d[0] = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
        d[1] = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
    }
}

__global__ __launch_bounds__(256) void dc_bn_finish_fwd_kernel(const double* __restrict__ part, int S, long long M, int C,
                                                               float* __restrict__ rm, float* __restrict__ rv,
                                                               long long* __restrict__ nbt, float* __restrict__ save) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int s = 0; s < S; ++s) { s0 += part[((size_t)s * C + c) * 2]; s1 += part[((size_t)s * C + c) * 2 + 1]; }
    const double mean = s0 / (double)M;
    double var = s1 / (double)M - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    save[c] = (float)mean;
    save[C + c] = (float)(1.0 / sqrt(var + 1e-5));
    if (rm) rm[c] = (float)(0.9 * (double)rm[c] + 0.1 * mean);
    if (rv) rv[c] = (float)(0.9 * (double)rv[c] + 0.1 * (var * (double)M / (double)(M - 1)));
    if (c == 0 && nbt) *nbt += 1;
}

__global__ __launch_bounds__(256) void dc_bn_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C,
                                                               float* __restrict__ save) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    save[c] = rm[c];
    save[C + c] = (float)(1.0 / sqrt((double)rv[c] + 1e-5));
}

__global__ __launch_bounds__(256) void dc_bn_apply_fwd_kernel(const float* __restrict__ x, const float* __restrict__ save,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, size_t n,
                                                              int C, float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const float xh = (x[i] - save[c]) * save[C + c];
    y[i] = dc_lrelu(xh * gamma[c] + beta[c]);
}

// coef [2 C] = (S1 / M | S2 / M) fp32; dbeta += S1, dgamma += S2
__global__ __launch_bounds__(256) void dc_bn_finish_bwd_kernel(const double* __restrict__ part, int S, long long M, int C,
                                                               float* __restrict__ coef, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int s = 0; s < S; ++s) { s0 += part[((size_t)s * C + c) * 2]; s1 += part[((size_t)s * C + c) * 2 + 1]; }
    coef[c] = (float)(s0 / (double)M);
    coef[C + c] = (float)(s1 / (double)M);
    if (dbeta) dbeta[c] += (float)s0;
    if (dgamma) dgamma[c] += (float)s1;
}

__global__ __launch_bounds__(256) void dc_bn_apply_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ save, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ coef, size_t n,
                                                              int C, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const float rstd = save[C + c], g = gamma[c];
    const float xh = (x[i] - save[c]) * rstd, z = xh * g + beta[c], dz = dy[i] * dc_lrelu_slope(z);
    dx[i] = (g * rstd) * ((dz - coef[c]) - xh * coef[C + c]);
}

__global__ __launch_bounds__(256) void dc_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y,
                                                       size_t n, int backward) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = backward ? dy[i] * dc_lrelu_slope(x[i]) : dc_lrelu(x[i]);
}

// ---- losses -----------------------------------------------------------------------------------------------------------------------
// (block partials through train_common.h's block_sum_d, folded by sums_begin / sums_end: pure fp64 adds)
template <bool DET>
__global__ __launch_bounds__(256) void dc_hinge_kernel(const float* __restrict__ real, const float* __restrict__ fake, size_t n, float factor,
                                                       float* __restrict__ dreal, float* __restrict__ dfake, double* __restrict__ out,
                                                       size_t nparts) {
    __shared__ double sh[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        const float r = real[i], f = fake[i], a = 1.f - r, b = 1.f + f;
        const float g = (float)(0.5 * (double)factor / (double)n);
        dreal[i] = a > 0.f ? -g : 0.f;
        dfake[i] = b > 0.f ? g : 0.f;
        v[0] = 0.5 * (double)factor * ((double)fmaxf(a, 0.f) + (double)fmaxf(b, 0.f)) / (double)n;
        v[1] = (double)r / (double)n;
        v[2] = (double)f / (double)n;
    }
    for (int k = 0; k < 3; ++k) {
        const double s = block_sum_d(v[k], sh);
        if (threadIdx.x == 0) {
            if constexpr (DET) out[(size_t)k * nparts + blockIdx.x] = s;
            else unsafeAtomicAdd(out + k, s);
        }
    }
}

template <bool DET>
__global__ __launch_bounds__(256) void dc_generator_kernel(const float* __restrict__ fake, size_t n, float* __restrict__ dfake,
                                                           double* __restrict__ out) {
    __shared__ double sh[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        dfake[i] = (float)(-1.0 / (double)n);
        v = -(double)fake[i] / (double)n;
    }
    v = block_sum_d(v, sh);
    if (threadIdx.x == 0) {
        if constexpr (DET) out[blockIdx.x] = v;
        else unsafeAtomicAdd(out, v);
    }
}

__global__ __launch_bounds__(256) void dc_adaptive_mix_kernel(const float* __restrict__ dnll, const float* __restrict__ dg,
                                                              const double* __restrict__ sq_nll, const double* __restrict__ sq_g,
                                                              float disc_weight, float disc_factor, float* __restrict__ dpred,
                                                              double* __restrict__ d_weight, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    double w = sqrt(*sq_nll) / (sqrt(*sq_g) + 1e-4);
    w = w < 0.0 ? 0.0 : (w > 1e4 ? 1e4 : w);                         // (a NaN stays a NaN, as torch.clamp's)
    w *= (double)disc_weight;
    if (i == 0) *d_weight = w;
    if (i >= n) return;
    const float s = (float)(w * (double)disc_factor);
    dpred[i] = dnll[i] + s * dg[i];
}

struct DcShape { int Wo, Ho; };
inline bool dc_shape(const rldm_train_disc_conv_desc* d, DcShape* s) {
    if (!d || d->B < 1 || d->Win < 2 || d->Hin < 2 || (d->stride != 1 && d->stride != 2)) return false;
    if (!(d->Cin == 2 || (d->Cin > 0 && d->Cin % 16 == 0)) || !(d->N == 1 || (d->N > 0 && d->N % 16 == 0))) return false;
    s->Wo = (d->Win - 2) / d->stride + 1;
    s->Ho = (d->Hin - 2) / d->stride + 1;
    // (pixel indices are ints)
    return (long long)d->B * d->Win * d->Hin < (1ll << 31) && (long long)d->B * s->Wo * s->Ho * 16 < (1ll << 31);
}

// K slices of the weight gradient: enough workgroups to fill the device, at least four 32-pixel chunks per slice, at most 64 slices
inline void dc_wgrad_plan(const rldm_train_disc_conv_desc* d, const DcShape& s, int* slices, int* cps) {
    const int tiles = ((d->N + 63) / 64) * ((d->Cin + 63) / 64) * 16;
    const int nchunks = (d->B * s.Wo * s.Ho + 31) / 32;
    int want = std::max(1, std::min({2048 / tiles, 64, nchunks / 4}));
    *cps = (nchunks + want - 1) / want;
    *slices = (nchunks + *cps - 1) / *cps;
}

}  // namespace

extern "C" {

int rldm_train_disc_conv_ok(const rldm_train_disc_conv_desc* d) {
    DcShape s;
    return dc_shape(d, &s) ? 1 : 0;
}

int rldm_train_disc_conv(const rldm_train_disc_conv_desc* d, const float* x, const void* w_packed, const float* bias, float* y,
                         void* stream) {
    DcShape s;
    RLDM_REQUIRE(dc_shape(d, &s), "rldm_train_disc_conv: no instance for this shape (Cin = 2 | 16 k, N = 1 | 16 k, stride 1 | 2, extents >= 2)");
    RLDM_REQUIRE(x && w_packed && y, "null argument");
    DcConv p{x, static_cast<const bf16_t*>(w_packed), bias, y, d->B, d->Win, d->Hin, d->Cin, (d->Cin + 15) / 16 * 16, s.Wo, s.Ho, d->N, 0,
             d->stride};
    const dim3 grid(((unsigned)(d->B * s.Wo * s.Ho) + 31) / 32, ((unsigned)d->N + 63) / 64, 1);
    if (d->Cin % 16 == 0) dc_conv_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    else dc_conv_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_disc_conv_dgrad(const rldm_train_disc_conv_desc* d, const float* dy, const void* w_transposed, float* dx, void* stream) {
    DcShape s;
    RLDM_REQUIRE(dc_shape(d, &s), "rldm_train_disc_conv_dgrad: no instance for this shape");
    RLDM_REQUIRE(dy && w_transposed && dx, "null argument");
    // the gathered tensor is dy [B][Wo][Ho][N], the produced one dx [B][Win][Hin][Cin]
    DcConv p{dy, static_cast<const bf16_t*>(w_transposed), nullptr, dx, d->B, s.Wo, s.Ho, d->N, (d->N + 15) / 16 * 16, d->Win, d->Hin,
             d->Cin, d->stride == 2 ? 2 : 1, d->stride};
    const unsigned P = d->stride == 2 ? (unsigned)(d->B * ((d->Win + 1) / 2) * ((d->Hin + 1) / 2)) : (unsigned)(d->B * d->Win * d->Hin);
    const dim3 grid((P + 31) / 32, ((unsigned)d->Cin + 63) / 64, d->stride == 2 ? 4 : 1);
    if (d->N % 16 == 0) dc_conv_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    else dc_conv_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p);
    TR_LAUNCH_CHECK();
    return 0;
}

int64_t rldm_train_disc_wgrad_workspace(const rldm_train_disc_conv_desc* d) {
    DcShape s;
    if (!dc_shape(d, &s)) return -1;
    int slices, cps;
    dc_wgrad_plan(d, s, &slices, &cps);
    return slices > 1 ? (int64_t)slices * d->N * d->Cin * 16 * (int64_t)sizeof(float) : 0;
}

int rldm_train_disc_wgrad(const rldm_train_disc_conv_desc* d, const float* dy, const float* x, float* dw, float* dbias,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    DcShape s;
    RLDM_REQUIRE(dc_shape(d, &s), "rldm_train_disc_wgrad: no instance for this shape");
    RLDM_REQUIRE(dy && x && dw, "null argument");
    int slices, cps;
    dc_wgrad_plan(d, s, &slices, &cps);
    const size_t n = (size_t)d->N * d->Cin * 16;
    RLDM_REQUIRE(slices == 1 || (workspace && workspace_bytes >= (int64_t)(slices * n * sizeof(float))),
                 "rldm_train_disc_wgrad: workspace smaller than rldm_train_disc_wgrad_workspace");
    hipStream_t st = (hipStream_t)stream;
    DcWgrad p{dy, x, slices == 1 ? dw : static_cast<float*>(workspace), d->B, d->Win, d->Hin, d->Cin, s.Wo, s.Ho, d->N, d->stride,
              d->B * s.Wo * s.Ho, cps, slices == 1 ? 1 : 0};
    const dim3 grid((unsigned)(((d->N + 63) / 64) * ((d->Cin + 63) / 64)), 16, (unsigned)slices);
    dc_wgrad_kernel<<<grid, 256, 0, st>>>(p);
    if (slices > 1) dc_wgrad_reduce_kernel<<<nblk(n), 256, 0, st>>>(static_cast<const float*>(workspace), slices, n, dw);
    TR_LAUNCH_CHECK();
    if (dbias) return rldm_train_colsum(dy, d->B, s.Wo * s.Ho, d->N, nullptr, 0, 0, dbias, stream);
    return 0;
}

int64_t rldm_train_disc_bn_workspace(int64_t M, int C) {
    if (M < 1 || C < 1) return -1;
    return ((M + 255) / 256) * C * 2 * (int64_t)sizeof(double) + (int64_t)C * 2 * (int64_t)sizeof(float);
}

int rldm_train_disc_bn_forward(const float* x, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, int training, float* save, float* y,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    RLDM_REQUIRE(x && gamma && beta && save && y, "null argument");
    RLDM_REQUIRE(M >= 1 && C >= 1 && M * C < (1ll << 40), "rldm_train_disc_bn_forward: M, C >= 1");
    hipStream_t st = (hipStream_t)stream;
    if (training) {
        RLDM_REQUIRE(M >= 2, "rldm_train_disc_bn_forward: expected more than 1 value per channel when training");
        RLDM_REQUIRE(workspace && workspace_bytes >= rldm_train_disc_bn_workspace(M, C),
                     "rldm_train_disc_bn_forward: workspace smaller than rldm_train_disc_bn_workspace");
        const int S = (int)((M + 255) / 256);
        double* part = static_cast<double*>(workspace);
        dc_bn_partial_kernel<false><<<dim3(((unsigned)C + 63) / 64, (unsigned)S), 256, 0, st>>>(x, nullptr, nullptr, nullptr, nullptr, M, C,
                                                                                                  part);
        dc_bn_finish_fwd_kernel<<<nblk((size_t)C), 256, 0, st>>>(part, S, M, C, running_mean, running_var,
                                                                 reinterpret_cast<long long*>(num_batches_tracked), save);
    } else {
        RLDM_REQUIRE(running_mean && running_var, "rldm_train_disc_bn_forward: eval mode needs the running statistics");
        dc_bn_eval_stats_kernel<<<nblk((size_t)C), 256, 0, st>>>(running_mean, running_var, C, save);
    }
    dc_bn_apply_fwd_kernel<<<nblk((size_t)M * C), 256, 0, st>>>(x, save, gamma, beta, (size_t)M * C, C, y);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_disc_bn_backward(const float* x, const float* dy, const float* save, int64_t M, int C, const float* gamma,
                                const float* beta, float* dx, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    RLDM_REQUIRE(x && dy && save && gamma && beta && dx, "null argument");
    RLDM_REQUIRE(M >= 2 && C >= 1 && M * C < (1ll << 40), "rldm_train_disc_bn_backward: M >= 2, C >= 1");
    RLDM_REQUIRE(workspace && workspace_bytes >= rldm_train_disc_bn_workspace(M, C),
                 "rldm_train_disc_bn_backward: workspace smaller than rldm_train_disc_bn_workspace");
    hipStream_t st = (hipStream_t)stream;
    const int S = (int)((M + 255) / 256);
    double* part = static_cast<double*>(workspace);
    float* coef = reinterpret_cast<float*>(part + (size_t)S * C * 2);
    dc_bn_partial_kernel<true><<<dim3(((unsigned)C + 63) / 64, (unsigned)S), 256, 0, st>>>(x, dy, save, gamma, beta, M, C, part);
    dc_bn_finish_bwd_kernel<<<nblk((size_t)C), 256, 0, st>>>(part, S, M, C, coef, dgamma, dbeta);
    dc_bn_apply_bwd_kernel<<<nblk((size_t)M * C), 256, 0, st>>>(x, dy, save, gamma, beta, coef, (size_t)M * C, C, dx);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_disc_lrelu(const float* x, const float* dy, float* y, int64_t n, int backward, void* stream) {
    RLDM_REQUIRE(x && y && n >= 0 && (!backward || dy), "null argument");
    if (n) dc_lrelu_kernel<<<nblk((size_t)n), 256, 0, (hipStream_t)stream>>>(x, dy, y, (size_t)n, backward);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_disc_hinge(const float* real, const float* fake, int64_t n, float factor, float* dreal, float* dfake, double* out,
                          double* partials, void* stream) {
    RLDM_REQUIRE(real && fake && dreal && dfake && out && n >= 1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nparts = nblk((size_t)n);
    const bool det = deterministic();
    RLDM_REQUIRE(!det || partials, "rldm_train_disc_hinge: the deterministic mode needs the partials buffer");
    double* dst = nullptr;
    if (sums_begin(det, 3, nparts, out, partials, st, &dst)) return 1;
    if (det) dc_hinge_kernel<true><<<nparts, 256, 0, st>>>(real, fake, (size_t)n, factor, dreal, dfake, dst, nparts);
    else dc_hinge_kernel<false><<<nparts, 256, 0, st>>>(real, fake, (size_t)n, factor, dreal, dfake, dst, nparts);
    return sums_end(det, 3, nparts, dst, out, st);
}

int rldm_train_disc_generator(const float* fake, int64_t n, float* dfake, double* out, double* partials, void* stream) {
    RLDM_REQUIRE(fake && dfake && out && n >= 1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nparts = nblk((size_t)n);
    const bool det = deterministic();
    RLDM_REQUIRE(!det || partials, "rldm_train_disc_generator: the deterministic mode needs the partials buffer");
    double* dst = nullptr;
    if (sums_begin(det, 1, nparts, out, partials, st, &dst)) return 1;
    if (det) dc_generator_kernel<true><<<nparts, 256, 0, st>>>(fake, (size_t)n, dfake, dst);
    else dc_generator_kernel<false><<<nparts, 256, 0, st>>>(fake, (size_t)n, dfake, dst);
    return sums_end(det, 1, nparts, dst, out, st);
}

int rldm_train_disc_adaptive_mix(const float* dnll, const float* dg, const double* sq_nll, const double* sq_g, float disc_weight,
                                 float disc_factor, float* dpred, double* d_weight, int64_t n, void* stream) {
    RLDM_REQUIRE(dnll && dg && sq_nll && sq_g && dpred && d_weight && n >= 1, "null argument");
    dc_adaptive_mix_kernel<<<nblk((size_t)n), 256, 0, (hipStream_t)stream>>>(dnll, dg, sq_nll, sq_g, disc_weight, disc_factor, dpred,
                                                                             d_weight, (size_t)n);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
