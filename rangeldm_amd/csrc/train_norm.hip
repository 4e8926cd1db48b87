// train_norm.hip -- GroupNorm(32) of the training step and the per-channel statistics of the fused tape (rldm_train_gn_forward,
// rldm_train_gn_backward, rldm_train_chan_stats, rldm_train_gn_backward_apply).  The arithmetic they share with the fused convs -- group
// moments, their two finishes, the backward element step -- is stated in train_common.h.
//   tr_gn_stats* / tr_gn_fwd*     (mean, rstd) per (image, group) and the forward (+ SiLU): a block per (image, group), or 64-pixel slabs
//   tr_gn_bwd_reduce* / _apply*   backward: the group sums with d gamma / d beta, then dx.
//   tr_chan_stats*                "cs" [B][C][2] = (sum, sum of squares) per (image, channel) for tensors no fused conv produced.
//   tr_gn_bwd_apply2_kernel       dx of a GroupNorm over a one- or two-source tensor from the dz and "gs" a fused data-gradient conv left.
#include "train_common.h"

using namespace rldm::train;

namespace {

// ---- GroupNorm ----------------------------------------------------------------------------------------------------------
// grid (groups, B): stats[b][g] = (mean, rstd) over npix x cpg values
__global__ __launch_bounds__(256) void tr_gn_stats_kernel(const float* __restrict__ x, int npix, int C, int groups, float eps,
                                                          float2* __restrict__ stats) {
    __shared__ double sh[4];
    const int g = blockIdx.x, b = blockIdx.y, cpg = C / groups;
    const float* base = x + (size_t)b * npix * C + g * cpg;
    double s = 0.0, ss = 0.0;
    for (int e = threadIdx.x; e < npix * cpg; e += 256) {
        const float v = base[(size_t)(e / cpg) * C + (e % cpg)];
        s += v;
        ss += (double)v * v;
    }
    s = block_sum_d(s, sh);
    ss = block_sum_d(ss, sh);
    if (threadIdx.x == 0) {
        const GnMoments m = gn_moments(s, ss, (double)npix * cpg);
        stats[b * groups + g] = make_float2((float)m.mean, gn_rstd_f64(m.var, eps));
    }
}

// Statistics AND apply in one launch for the small tensors (levels 1-3): the block of (image, group) re-reads its own slab
// (it is 2-32 KB: L1 / L2 hits) and writes y.  Saves a launch per GroupNorm where a launch costs more than the work.
__global__ __launch_bounds__(256) void tr_gn_fwd_fused_vec_kernel(const float* __restrict__ x, int npix, int C, int groups, float eps,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  int silu, float2* __restrict__ stats, float* __restrict__ y) {
    __shared__ double sh[4];
    __shared__ float2 sst;
    const int g = blockIdx.x, b = blockIdx.y, cpg = C / groups, Q = cpg >> 2;
    const int q = threadIdx.x % Q, pl = threadIdx.x / Q, step = 256 / Q;
    const size_t off = (size_t)b * npix * C + g * cpg + 4 * q;
    double s = 0.0, ss = 0.0;
    for (int p = pl; p < npix; p += step) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + off + (size_t)p * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) { s += v[e]; ss += (double)v[e] * v[e]; }
    }
    s = block_sum_d(s, sh);
    ss = block_sum_d(ss, sh);
    if (threadIdx.x == 0) {
        const GnMoments m = gn_moments(s, ss, (double)npix * cpg);
        sst = make_float2((float)m.mean, gn_rstd_f64(m.var, eps));
        stats[b * groups + g] = sst;
    }
    __syncthreads();
    const float2 st = sst;
    const f32x4 ga = tr_load4(gamma + g * cpg + 4 * q), be = tr_load4(beta + g * cpg + 4 * q);
    for (int p = pl; p < npix; p += step) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + off + (size_t)p * C);
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float z = (v[e] - st.x) * st.y * ga[e] + be[e];
            out[e] = silu ? z * sigmoid_f(z) : z;
        }
        *reinterpret_cast<f32x4*>(y + off + (size_t)p * C) = out;
    }
}

// Large tensors: the one-block-per-(image, group) kernels above read 16-byte pieces 2 KB apart.  These variants give a
// block a slab of 64 pixels x all channels (fully coalesced float4 rows); a thread's channel quad is the same in every
// iteration when C divides 1024, so it accumulates in registers and ends with one LDS atomic per group it touched.
// acc [B][groups][2] doubles (zeroed by the caller): (sum, sum of squares).
__global__ __launch_bounds__(256) void tr_gn_stats_slab_kernel(const float* __restrict__ x, int npix, int C, int groups,
                                                               double* __restrict__ acc) {
    __shared__ double sS[64], sSS[64];
    const int b = blockIdx.y, cpg = C / groups;
    const int p0 = blockIdx.x * 64, p1 = min(p0 + 64, npix);
    if (threadIdx.x < groups) { sS[threadIdx.x] = 0.0; sSS[threadIdx.x] = 0.0; }
    __syncthreads();
    const float4* base = reinterpret_cast<const float4*>(x + ((size_t)b * npix + p0) * C);
    const int n4 = (p1 - p0) * C / 4;
    const int c0 = (threadIdx.x * 4) % C;                  // fixed channel quad (C divides 1024)
    float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 v = base[i];
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        ss[0] += v.x * v.x; ss[1] += v.y * v.y; ss[2] += v.z * v.z; ss[3] += v.w * v.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = (c0 + e) / cpg;
        atomicAdd(&sS[g], (double)s[e]);
        atomicAdd(&sSS[g], (double)ss[e]);
    }
    __syncthreads();
    if (threadIdx.x < groups) {
        unsafeAtomicAdd(acc + ((size_t)b * groups + threadIdx.x) * 2, sS[threadIdx.x]);
        unsafeAtomicAdd(acc + ((size_t)b * groups + threadIdx.x) * 2 + 1, sSS[threadIdx.x]);
    }
}

// (the finish kernels leave the accumulators zeroed for the next launch: no separate fill)
__global__ __launch_bounds__(256) void tr_gn_stats_finish_kernel(double* __restrict__ acc, int n, double count, float eps,
                                                                 float2* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double s0 = acc[2 * i], s1 = acc[2 * i + 1];
    acc[2 * i] = 0.0;
    acc[2 * i + 1] = 0.0;
    const GnMoments m = gn_moments(s0, s1, count);
    stats[i] = make_float2((float)m.mean, gn_rstd_f64(m.var, eps));
}


__global__ __launch_bounds__(256) void tr_gn_fwd_kernel(const float* __restrict__ x, const float2* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, int npix,
                                                        int C, int groups, int silu, size_t total, float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int b = (int)(i / ((size_t)npix * C));
    const float2 st = stats[b * groups + c / (C / groups)];
    const float z = (x[i] - st.x) * st.y * gamma[c] + beta[c];
    y[i] = silu ? z * sigmoid_f(z) : z;
}

// four channels per thread (channels per group a multiple of 4, fewer than 2^31 elements): 16-byte accesses, 32-bit index math
__global__ __launch_bounds__(256) void tr_gn_fwd_vec_kernel(const float* __restrict__ x, const float2* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            unsigned per_image, unsigned C, unsigned cpg, int groups, int silu,
                                                            unsigned total4, float* __restrict__ y) {
    const unsigned i4 = blockIdx.x * 256 + threadIdx.x;
    if (i4 >= total4) return;
    const unsigned i = i4 * 4, c = i % C, b = i / per_image;
    const float2 st = stats[b * groups + c / cpg];
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
    const f32x4 ga = tr_load4(gamma + c), be = tr_load4(beta + c);
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float z = (xv[e] - st.x) * st.y * ga[e] + be[e];
        out[e] = silu ? z * sigmoid_f(z) : z;
    }
    *reinterpret_cast<f32x4*>(y + i) = out;
}

__global__ __launch_bounds__(256) void tr_gn_bwd_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const float2* __restrict__ stats, const float2* __restrict__ sums,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  unsigned per_image, unsigned C, unsigned cpg, int groups, int silu,
                                                                  int accumulate, float inv_n, unsigned total4, float* __restrict__ dx) {
    const unsigned i4 = blockIdx.x * 256 + threadIdx.x;
    if (i4 >= total4) return;
    const unsigned i = i4 * 4, c = i % C, b = i / per_image;
    const int sg_i = b * groups + c / cpg;
    const float2 st = stats[sg_i], sm = sums[sg_i];
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i), dv = *reinterpret_cast<const f32x4*>(dy + i);
    const f32x4 ga = tr_load4(gamma + c), be = tr_load4(beta + c);
    f32x4 out;
    if (accumulate) out = *reinterpret_cast<const f32x4*>(dx + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const auto [xh, dz] = gn_bwd_elem(xv[e], dv[e], st.x, st.y, ga[e], be[e], silu);
        const float v = st.y * (dz * ga[e] - sm.x * inv_n - xh * sm.y * inv_n);
        out[e] = accumulate ? out[e] + v : v;
    }
    *reinterpret_cast<f32x4*>(dx + i) = out;
}

// grid (groups, B): sums[b][g] = (sum dz gamma, sum dz gamma xhat); dgamma[c] += sum dz xhat, dbeta[c] += sum dz
// (dz = dy * act'(z)); the first T = 256 - 256 % cpg threads stride by T, so thread t always meets channel t % cpg
// DET (rldm_train_deterministic): dgamma / dbeta = partial rows [B][C], added over the images in image order by tr_fold_rows_kernel
template <bool DET = false>
__global__ __launch_bounds__(256) void tr_gn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int npix, int C, int groups, int silu,
                                                               float2* __restrict__ sums, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
    __shared__ double sh[4];
    __shared__ float shg[256], shb[256];
    const int g = blockIdx.x, b = blockIdx.y, cpg = C / groups;
    const float2 st = stats[b * groups + g];
    const size_t base = (size_t)b * npix * C + g * cpg;
    const int ci = threadIdx.x % cpg, c = g * cpg + ci;
    const int TT = 256 - 256 % cpg;
    const float ga = gamma[c], be = beta[c];
    double s1 = 0.0, s2 = 0.0;
    float dg = 0.f, db = 0.f;
    for (int e = threadIdx.x < TT ? threadIdx.x : npix * cpg; e < npix * cpg; e += TT) {
        const size_t idx = base + (size_t)(e / cpg) * C + ci;
        const auto [xh, dz] = gn_bwd_elem(x[idx], dy[idx], st.x, st.y, ga, be, silu);
        s1 += (double)(dz * ga);
        s2 += (double)(dz * ga * xh);
        dg += dz * xh;
        db += dz;
    }
    s1 = block_sum_d(s1, sh);
    s2 = block_sum_d(s2, sh);
    shg[threadIdx.x] = dg;
    shb[threadIdx.x] = db;
    __syncthreads();
    if (threadIdx.x < cpg) {
        float tg = 0.f, tb = 0.f;
        for (int t = threadIdx.x; t < TT; t += cpg) { tg += shg[t]; tb += shb[t]; }
        if constexpr (DET) {
            dgamma[(size_t)b * C + g * cpg + threadIdx.x] = tg;
            dbeta[(size_t)b * C + g * cpg + threadIdx.x] = tb;
        } else {
            unsafeAtomicAdd(dgamma + g * cpg + threadIdx.x, tg);
            unsafeAtomicAdd(dbeta + g * cpg + threadIdx.x, tb);
        }
    }
    if (threadIdx.x == 0) sums[b * groups + g] = make_float2((float)s1, (float)s2);
}

// slab variant of the reduction (see tr_gn_stats_slab_kernel): acc [B][groups][2] doubles = (sum dz gamma, sum dz gamma xhat);
// dgamma / dbeta by one global atomic per channel and block
__global__ __launch_bounds__(256) void tr_gn_bwd_reduce_slab_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    const float2* __restrict__ stats, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, int npix, int C, int groups,
                                                                    int silu, double* __restrict__ acc, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta) {
    __shared__ double s1[64], s2[64];
    __shared__ float sg[1024], sb[1024];
    const int b = blockIdx.y, cpg = C / groups;
    const int SP = gridDim.z ? (npix + gridDim.x - 1) / gridDim.x : 64;   // pixels per block (the launcher's slab size)
    const int p0 = blockIdx.x * SP, p1 = min(p0 + SP, npix);
    if (threadIdx.x < groups) { s1[threadIdx.x] = 0.0; s2[threadIdx.x] = 0.0; }
    for (int c = threadIdx.x; c < C; c += 256) { sg[c] = 0.f; sb[c] = 0.f; }
    __syncthreads();
    const size_t off = ((size_t)b * npix + p0) * C;
    const float4* bx = reinterpret_cast<const float4*>(x + off);
    const float4* bd = reinterpret_cast<const float4*>(dy + off);
    const int n4 = (p1 - p0) * C / 4;
    const int c0 = (threadIdx.x * 4) % C;
    float ga[4], be[4], mean[4], rstd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float2 st = stats[b * groups + (c0 + e) / cpg];
        ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; mean[e] = st.x; rstd[e] = st.y;
    }
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f}, dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 xv = bx[i], dv = bd[i];
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w}, de[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const auto [xh, dz] = gn_bwd_elem(xe[e], de[e], mean[e], rstd[e], ga[e], be[e], silu);
            a1[e] += dz * ga[e];
            a2[e] += dz * ga[e] * xh;
            dg[e] += dz * xh;
            db[e] += dz;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = (c0 + e) / cpg;
        atomicAdd(&s1[g], (double)a1[e]);
        atomicAdd(&s2[g], (double)a2[e]);
        atomicAdd(&sg[c0 + e], dg[e]);
        atomicAdd(&sb[c0 + e], db[e]);
    }
    __syncthreads();
    if (threadIdx.x < groups) {
        unsafeAtomicAdd(acc + ((size_t)b * groups + threadIdx.x) * 2, s1[threadIdx.x]);
        unsafeAtomicAdd(acc + ((size_t)b * groups + threadIdx.x) * 2 + 1, s2[threadIdx.x]);
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        unsafeAtomicAdd(dgamma + c, sg[c]);
        unsafeAtomicAdd(dbeta + c, sb[c]);
    }
}

__global__ __launch_bounds__(256) void tr_gn_sums_finish_kernel(double* __restrict__ acc, int n, float2* __restrict__ sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    sums[i] = make_float2((float)acc[2 * i], (float)acc[2 * i + 1]);
    acc[2 * i] = 0.0;
    acc[2 * i + 1] = 0.0;
}

__global__ __launch_bounds__(256) void tr_gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float2* __restrict__ stats, const float2* __restrict__ sums,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              int npix, int C, int groups, int silu, int accumulate, size_t total,
                                                              float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), cpg = C / groups;
    const int b = (int)(i / ((size_t)npix * C));
    const int sg_i = b * groups + c / cpg;
    const float2 st = stats[sg_i], sm = sums[sg_i];
    const auto [xh, dz] = gn_bwd_elem(x[i], dy[i], st.x, st.y, gamma[c], beta[c], silu);
    const float inv_n = 1.f / ((float)npix * cpg);
    const float v = st.y * (dz * gamma[c] - sm.x * inv_n - xh * sm.y * inv_n);
    dx[i] = accumulate ? dx[i] + v : v;
}

// ---- (round 5) per-channel statistics and the GroupNorm backward apply of the fused tape -------------------------------------
// cs[b][c] += (sum, sum of squares) over a slab of image b's pixels: for tensors no fused conv produced (conv_in's output).
// grid (slabs, B); thread (pixel lane t / Q, channel quad t % Q), Q = C / 4 <= 256.
__global__ __launch_bounds__(256) void tr_chan_stats_kernel(const float* __restrict__ x, int npix, int C, int slab, float* __restrict__ cs) {
    __shared__ float sacc[2 * 1024];
    const int b = blockIdx.y, Q = C >> 2, step = 256 / Q;
    const int q = threadIdx.x % Q, pl = threadIdx.x / Q;
    for (int e = threadIdx.x; e < 2 * C; e += 256) sacc[e] = 0.f;
    __syncthreads();
    if (pl < step) {
        const int p0 = blockIdx.x * slab, p1 = min(p0 + slab, npix);
        const float* base = x + (size_t)b * npix * C + 4 * q;
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, ss = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int px = p0 + pl; px < p1; px += step) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(base + (size_t)px * C);
            s += v;
            ss += v * v;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(&sacc[(4 * q + e) * 2], s[e]);
            atomicAdd(&sacc[(4 * q + e) * 2 + 1], ss[e]);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += 256) unsafeAtomicAdd(cs + (size_t)b * C * 2 + e, sacc[e]);
}

// (deterministic mode) the canonical partials of the GroupNorm statistics (include/rangeldm_hip.h, rldm_train_deterministic): partial t
// of image b covers pixels [64 t, 64 t + 64); lane k of 16 adds x (and the rounded x * x) of pixels 64 t + k + 16 j, j = 0 .. 3, in
// that order; the lanes are added k = 0 .. 15: exactly what tr_tile_epilogue<BN, true> leaves for the tile a fused conv stored.
// part [B][T][C][2]; grid (T, B, C / 64 rounded up), thread (lane tid / 16, channel quad tid % 16).
__global__ __launch_bounds__(256) void tr_chan_stats_det_kernel(const float* __restrict__ x, int npix, int C, float* __restrict__ part) {
    __shared__ float lanes[16][128];
    const int t = blockIdx.x, b = blockIdx.y, k = threadIdx.x >> 4, cq = threadIdx.x & 15;
    const int ch = blockIdx.z * 64 + 4 * cq;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, ss = {0.f, 0.f, 0.f, 0.f};
    if (ch < C) {                                                   // (C % 4 == 0: a quad is inside or outside)
        const float* base = x + (size_t)b * npix * C + ch;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int px = 64 * t + k + 16 * j;
            if (px < npix) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(base + (size_t)px * C);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s[q] = det_add(s[q], v[q]);
                    ss[q] = det_add(ss[q], det_mul(v[q], v[q]));
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lanes[k][2 * (4 * cq + q)] = s[q];
        lanes[k][2 * (4 * cq + q) + 1] = ss[q];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c2 = blockIdx.z * 64 + (threadIdx.x >> 1);
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) a = det_add(a, lanes[r][threadIdx.x]);
        if (c2 < C) part[(((size_t)b * gridDim.x + t) * C + c2) * 2 + (threadIdx.x & 1)] = a;
    }
}

// dx = rstd (gamma dz - s1 / n - xhat s2 / n) [+ res] of a GroupNorm over cat(x0, x1), from dz = dy act'(z) (stored by the data-gradient
// conv's epilogue) and gs[b][c] = (sum dz, sum dz xhat): s1 = sum over the group of gamma gs.x, s2 = ... gamma gs.y.  The result is
// written (or added) to the two sources' gradients separately; d gamma / d beta are finished by block (0, 0).  grid (slabs, B).
struct TrGnApply {
    const float* dz; const float* x0; const float* x1; const float* cs0; const float* cs1; const float* gs; const float* gamma;
    const float* res; float* dx0; float* dx1; float* dgamma; float* dbeta;
    int B, npix, C, C0, groups, slab, acc0, acc1; float eps;
};
__global__ __launch_bounds__(256) void tr_gn_bwd_apply2_kernel(const TrGnApply a) {
    __shared__ float4 sT[768];                  // per channel: (rstd gamma, rstd s1 / n, rstd s2 / n, -)
    __shared__ float2 sM[768];                  // per channel: (mean, rstd)
    __shared__ float4 sG[64];                   // per group: (mean, rstd, s1, s2)
    const int tid = threadIdx.x, b = blockIdx.y, C = a.C, C0 = a.C0, C1 = C - C0, cpg = C / a.groups;
    for (int c = tid; c < C; c += 256) {
        const float2 v = c < C0 ? reinterpret_cast<const float2*>(a.cs0)[(size_t)b * C0 + c] : reinterpret_cast<const float2*>(a.cs1)[(size_t)b * C1 + c - C0];
        const float2 g = reinterpret_cast<const float2*>(a.gs)[(size_t)b * C + c];
        const float ga = a.gamma[c];
        sM[c] = v;
        sT[c] = make_float4(ga, g.x * ga, g.y * ga, 0.f);
    }
    __syncthreads();
    const double n = (double)a.npix * cpg;
    for (int g = tid; g < a.groups; g += 256) {
        double s = 0.0, ss = 0.0, s1 = 0.0, s2 = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { s += (double)sM[c].x; ss += (double)sM[c].y; s1 += (double)sT[c].y; s2 += (double)sT[c].z; }
        const GnMoments m = gn_moments(s, ss, n);
        sG[g] = make_float4((float)m.mean, gn_rstd_f64(m.var, a.eps), (float)(s1 / n), (float)(s2 / n));
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float4 g = sG[c / cpg];
        const float ga = sT[c].x;
        sM[c] = make_float2(g.x, g.y);
        sT[c] = make_float4(g.y * ga, g.y * g.z, g.y * g.w, 0.f);
    }
    __syncthreads();
    if (blockIdx.x == 0 && b == 0 && a.dgamma)
        for (int c = tid; c < C; c += 256) {
            float dg = 0.f, db = 0.f;
            for (int bi = 0; bi < a.B; ++bi) {
                const float2 g = reinterpret_cast<const float2*>(a.gs)[(size_t)bi * C + c];
                db += g.x; dg += g.y;
            }
            a.dgamma[c] += dg;
            a.dbeta[c] += db;
        }
    const int p0 = blockIdx.x * a.slab, p1 = min(p0 + a.slab, a.npix);
    const int Q = C >> 2, n4 = (p1 - p0) * Q;
    const size_t pix0 = (size_t)b * a.npix + p0;
    for (int i = tid; i < n4; i += 256) {
        const int pl = i / Q, c = (i - pl * Q) * 4;
        const size_t px = pix0 + pl;
        const f32x4 dz = *reinterpret_cast<const f32x4*>(a.dz + px * C + c);
        const bool first = c < C0;
        const size_t off = first ? px * C0 + c : px * C1 + (c - C0);
        const f32x4 xv = *reinterpret_cast<const f32x4*>((first ? a.x0 : a.x1) + off);
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 t = sT[c + e];
            const float2 m = sM[c + e];
            out[e] = t.x * dz[e] - t.y - (xv[e] - m.x) * m.y * t.z;
        }
        if (a.res) out += *reinterpret_cast<const f32x4*>(a.res + px * C + c);
        float* dst = (first ? a.dx0 : a.dx1) + off;
        if (first ? a.acc0 : a.acc1) out += *reinterpret_cast<const f32x4*>(dst);
        *reinterpret_cast<f32x4*>(dst) = out;
    }
}

}  // namespace

extern "C" {

// fp64 accumulators of the slab GroupNorm kernels: zeroed once, every user leaves them zeroed (finish kernels)
static int gn_accumulators(size_t count, hipStream_t st, double** out) {
    return tr_scratch(kGnAccumulators, count * sizeof(double), 4096 * sizeof(double), true, st, reinterpret_cast<void**>(out));
}

int rldm_train_gn_forward(const float* x, int B, int npix, int C, int groups, float eps, const float* gamma, const float* beta,
                          int silu, float* stats, float* y, void* stream) {
    RLDM_REQUIRE(x && gamma && beta && stats && y, "null argument");
    RLDM_REQUIRE(C % groups == 0, "channels must be a multiple of the group count");
    hipStream_t st = (hipStream_t)stream;
    // (deterministic mode: the slab kernels meet in atomics; the one-block-per-(image, group) kernels add in a fixed order)
    const bool slab = !deterministic() && 1024 % C == 0 && C >= 4 && groups <= 64 && (size_t)npix * C >= (1u << 18);     // large tensors, see the kernel
    if (slab) {
        double* acc = nullptr;
        if (gn_accumulators((size_t)B * groups * 2, st, &acc)) return 1;
        tr_gn_stats_slab_kernel<<<dim3((npix + 63) / 64, B), 256, 0, st>>>(x, npix, C, groups, acc);
        tr_gn_stats_finish_kernel<<<nblk((size_t)B * groups), 256, 0, st>>>(acc, B * groups, (double)npix * (C / groups), eps,
                                                                           reinterpret_cast<float2*>(stats));
    } else if ((C / groups) % 4 == 0 && C / groups <= 16 && (C / groups & (C / groups - 1)) == 0) {
        tr_gn_fwd_fused_vec_kernel<<<dim3(groups, B), 256, 0, st>>>(x, npix, C, groups, eps, gamma, beta, silu,
                                                                    reinterpret_cast<float2*>(stats), y);
        TR_LAUNCH_CHECK();
        return 0;
    } else
        tr_gn_stats_kernel<<<dim3(groups, B), 256, 0, st>>>(x, npix, C, groups, eps, reinterpret_cast<float2*>(stats));
    const size_t total = (size_t)B * npix * C;
    const int cpg = C / groups;
    if (cpg % 4 == 0 && total < (1ull << 31))
        tr_gn_fwd_vec_kernel<<<nblk(total / 4), 256, 0, st>>>(x, reinterpret_cast<const float2*>(stats), gamma, beta, (unsigned)npix * C, C,
                                                            cpg, groups, silu, (unsigned)(total / 4), y);
    else
        tr_gn_fwd_kernel<<<nblk(total), 256, 0, st>>>(x, reinterpret_cast<const float2*>(stats), gamma, beta, npix, C, groups, silu, total, y);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_gn_backward(const float* x, const float* dy, const float* stats, int B, int npix, int C, int groups,
                           const float* gamma, const float* beta, int silu, float* scratch, float* dx, int accumulate,
                           float* dgamma, float* dbeta, void* stream) {
    RLDM_REQUIRE(x && dy && stats && gamma && beta && scratch && dx && dgamma && dbeta, "null argument");
    RLDM_REQUIRE(C % groups == 0 && C / groups <= 256, "channels per group must be <= 256");
    hipStream_t st = (hipStream_t)stream;
    const bool slab = !deterministic() && 1024 % C == 0 && C >= 4 && C <= 1024 && groups <= 64 && (size_t)npix * C >= (1u << 18);
    if (deterministic()) {
        float* part = nullptr;                      // [2][B][C]: d gamma, d beta per image
        if (det_partials((size_t)2 * B * C * sizeof(float), st, reinterpret_cast<void**>(&part))) return 1;
        tr_gn_bwd_reduce_kernel<true><<<dim3(groups, B), 256, 0, st>>>(x, dy, reinterpret_cast<const float2*>(stats), gamma, beta, npix, C,
                                                                       groups, silu, reinterpret_cast<float2*>(scratch), part,
                                                                       part + (size_t)B * C);
        if (launch_fold_rows(part, 1, B, C, dgamma, C, 1, st) || launch_fold_rows(part + (size_t)B * C, 1, B, C, dbeta, C, 1, st)) return 1;
    } else if (slab) {
        double* acc = nullptr;
        if (gn_accumulators((size_t)B * groups * 2, st, &acc)) return 1;
        constexpr int kSlab = 64;                   // pixels per block
        tr_gn_bwd_reduce_slab_kernel<<<dim3((npix + kSlab - 1) / kSlab, B), 256, 0, st>>>(x, dy, reinterpret_cast<const float2*>(stats), gamma,
                                                                               beta, npix, C, groups, silu, acc, dgamma, dbeta);
        tr_gn_sums_finish_kernel<<<nblk((size_t)B * groups), 256, 0, st>>>(acc, B * groups, reinterpret_cast<float2*>(scratch));
    } else
        // (a four-channels-per-thread form measured 14.0 us against this kernel's 10.1: four sigmoids per iteration and the wider
        //  LDS epilogue cost more than the 16-byte loads save)
        tr_gn_bwd_reduce_kernel<false><<<dim3(groups, B), 256, 0, st>>>(x, dy, reinterpret_cast<const float2*>(stats), gamma, beta, npix, C,
                                                                 groups, silu, reinterpret_cast<float2*>(scratch), dgamma, dbeta);
    const size_t total = (size_t)B * npix * C;
    if ((C / groups) % 4 == 0 && total < (1ull << 31))
        tr_gn_bwd_apply_vec_kernel<<<nblk(total / 4), 256, 0, st>>>(x, dy, reinterpret_cast<const float2*>(stats),
                                                                  reinterpret_cast<const float2*>(scratch), gamma, beta, (unsigned)npix * C,
                                                                  C, C / groups, groups, silu, accumulate,
                                                                  1.f / ((float)npix * (C / groups)), (unsigned)(total / 4), dx);
    else
        tr_gn_bwd_apply_kernel<<<nblk(total), 256, 0, st>>>(x, dy, reinterpret_cast<const float2*>(stats),
                                                        reinterpret_cast<const float2*>(scratch), gamma, beta, npix, C, groups, silu,
                                                        accumulate, total, dx);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_chan_stats(const float* x, int B, int npix, int C, float* cs, void* stream) {
    RLDM_REQUIRE(x && cs && B > 0 && npix > 0, "null argument");
    RLDM_REQUIRE(C % 4 == 0 && C <= 1024, "channels: a multiple of 4, <= 1024");
    if (deterministic()) {
        hipStream_t st = (hipStream_t)stream;
        const int T = (npix + 63) / 64;
        float* part = nullptr;
        if (det_partials((size_t)B * T * C * 2 * sizeof(float), st, reinterpret_cast<void**>(&part))) return 1;
        tr_chan_stats_det_kernel<<<dim3(T, B, (C + 63) / 64), 256, 0, st>>>(x, npix, C, part);
        return launch_fold_rows(part, B, T, 2 * C, cs, 2 * C, 1, st);
    }
    const int slab = npix >= 4096 ? 256 : 64;
    tr_chan_stats_kernel<<<dim3((npix + slab - 1) / slab, B), 256, 0, (hipStream_t)stream>>>(x, npix, C, slab, cs);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_gn_backward_apply(const float* dz, const float* x0, const float* x1, int C0, const float* cs0, const float* cs1,
                                 const float* gs, int B, int npix, int C, int groups, float eps, const float* gamma, const float* res,
                                 float* dx0, int accumulate0, float* dx1, int accumulate1, float* dgamma, float* dbeta, void* stream) {
    RLDM_REQUIRE(dz && x0 && cs0 && gs && gamma && dx0, "null argument");
    RLDM_REQUIRE(C % 4 == 0 && C <= 768 && groups >= 1 && groups <= 64 && C % groups == 0, "channels: a multiple of 4 and of the groups, <= 768");
    RLDM_REQUIRE(!x1 || (cs1 && dx1 && C0 > 0 && C0 < C && C0 % 4 == 0), "two sources: C0 a multiple of 4 inside (0, C)");
    RLDM_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "d gamma and d beta come together");
    TrGnApply a;
    a.dz = dz; a.x0 = x0; a.x1 = x1; a.cs0 = cs0; a.cs1 = cs1; a.gs = gs; a.gamma = gamma; a.res = res; a.dx0 = dx0; a.dx1 = dx1;
    a.dgamma = dgamma; a.dbeta = dbeta; a.B = B; a.npix = npix; a.C = C; a.C0 = x1 ? C0 : C; a.groups = groups;
    a.acc0 = accumulate0; a.acc1 = accumulate1; a.eps = eps;
    // slabs of >= 16 pixels, ~1024 blocks at most
    int slab = 16;
    while ((long long)B * ((npix + slab - 1) / slab) > 512) slab *= 2;
    a.slab = slab;
    tr_gn_bwd_apply2_kernel<<<dim3((npix + slab - 1) / slab, B), 256, 0, (hipStream_t)stream>>>(a);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
