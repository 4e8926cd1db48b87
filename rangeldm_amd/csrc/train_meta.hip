// The range-guided Meta-Kernel layer of the KITTI-360 discriminator (include/rangeldm_hip.h: rldm_train_meta_*; reference: MetaKernel
// and NLayerDiscriminatorMetaKernel, vae/sgm/modules/autoencoding/lpips/model/model.py:91-265), forward and all three gradients.
//
// Tensors are NHWC [B][W][H][C] fp32; a ROW is one (output pixel, tap) pair, row = 16 px + t, t = 4 i + j (i: shift along H, j: shift
// along W, W wraps, outside H the features read 0 and the range reads 100).  Everything row-shaped is laid out [row][channel], so the
// modulated patch of a pixel is [t][c] (K index t C + c) where the reference's coov weight is [c][t]: the GEMMs below read and write
// that weight through an index map instead of a packed copy.
//
//   forward   mk_pe_kernel            pe [row][3], the source pixel of every row, the next layer's r (the centre tap)
//             mk_gemm (hidden A)      m = r(h) r(W2)^T + b2, h = lrelu(W1 pe + b1) made in fp32 while the tile is staged
//             mk_gemm (modulated A)   y = r(m x_patch) r(coov)^T + bias, the modulated patch made while the tile is staged
//   backward  mk_gemm                 G = r(dy) r(coov);  dcoov += r(dy)^T r(m x_patch);  dh = r(dm) r(W2);  dW2 += r(dm)^T r(h)
//             mk_dx_kernel            dx = the gather of G m over the rows that read a pixel
//             mk_dm_kernel            dm = G x_patch (in place);  mk_mask_kernel: dpre = dh lrelu'(pre) (in place)
//             mk_gemm (fp32)          dW1 += dpre^T pe;  dpe = dpre W1;  and the whole MLP of the C = 2 layer
//             mk_dr_kernel            dr = the gather of dpe through both roles of a pixel (tap, centre) + the next layer's dr
// r(.) is rounding to bf16 on the way into LDS; both operands of every MFMA (32x32x16 bf16, fp32 accumulation) are staged there by the
// whole workgroup.  The fp32 instance of the same kernel multiplies and adds on the VALU (k in order).  No kernel of this file uses
// an atomic: a reduction dimension that is cut into slices leaves partial tiles that are added in slice order, in both modes of
// rldm_train_deterministic.  The three bias sums are rldm_train_colsum's (fp32 atomics in the default mode, ordered in the other).  The arithmetic is restated in rangeldm_amd/metakernel.py (*_host): no FMA contraction
// in this file.
#include "common.h"
#include "../../include/rangeldm_hip.h"

#include <algorithm>
#include <cstdint>

namespace {

typedef long long i64;

inline unsigned mk_nblk(i64 n) { return (unsigned)((n + 255) / 256); }

__device__ __forceinline__ float mk_lrelu(float z) { return z > 0.f ? z : 0.2f * z; }
__device__ __forceinline__ float mk_slope(float z) { return z > 0.f ? 1.f : 0.2f; }

struct MkGeom { int B, W, H, C, N, s, Wo, Ho; };

// ---- positional encoding ---------------------------------------------------------------------------------------------------------
// tables [4][16] = cos_azi | sin_azi | cos_inc | sin_inc, each [i][j]
__global__ __launch_bounds__(256) void mk_pe_kernel(const MkGeom g, const float* __restrict__ r, const float* __restrict__ tab,
                                                    float* __restrict__ pe, int* __restrict__ src, float* __restrict__ r_next) {
    const i64 row = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 R = (i64)g.B * g.Wo * g.Ho * 16;
    if (row >= R) return;
    const int t = (int)(row & 15), i = t >> 2, j = t & 3;
    const i64 px = row >> 4;
    const int ho = (int)(px % g.Ho), wo = (int)((px / g.Ho) % g.Wo), b = (int)(px / ((i64)g.Ho * g.Wo));
    const int w = (g.s * wo + j - 1 + g.W) % g.W, h = g.s * ho + i - 1;
    const bool in = h >= 0 && h < g.H;
    const int sp = in ? (b * g.W + w) * g.H + h : -1;
    const float rc = r[((i64)b * g.W + (g.s * wo + 1) % g.W) * g.H + g.s * ho + 1];
    const float rt = in ? r[sp] : 100.f;
    const float a = rt * tab[t];
    pe[row * 3 + 0] = a * tab[32 + t] - rc;
    pe[row * 3 + 1] = a * tab[48 + t];
    pe[row * 3 + 2] = rt * tab[16 + t];
    src[row] = sp;
    if (t == 10 && r_next) r_next[px] = rc;
}

// ---- the GEMM --------------------------------------------------------------------------------------------------------------------
// out[m][n] (+)= sum_k A(m, k) B(n, k) (+ bias[n]).  An operand element is read through its loader:
//   PLAIN      p[f_o(u) + f_k(k)], f(v) = v lo, or (v / D) hi + (v % D) lo for the coov weight's [c][t] order (D = C, hi = 1, lo = 16)
//   HIDDEN     h(row, c) = lrelu(((W1[c][0] pe0 + W1[c][1] pe1) + W1[c][2] pe2) + b1[c])
//   MODULATED  m[row][c] x[src[row]][c] (0 where the row's source is outside H), (px, j) -> row = 16 px + j / C, c = j % C
// For HIDDEN / MODULATED `swap` says that the reduction index is the row (pixel) and the outer one the channel (j).
struct MkIdx { i64 D, hi, lo; };
// (D == 0: the linear map v lo, no division; the permuted coov index has D = C and v < 16 C, 32-bit arithmetic)
__host__ __device__ inline i64 mk_at(const MkIdx& f, i64 v) {
    if (f.D == 0) return v * f.lo;
    const unsigned u = (unsigned)v, d = (unsigned)f.D;
    return (i64)(u / d) * f.hi + (i64)(u % d) * f.lo;
}
inline MkIdx mk_lin(i64 stride) { return MkIdx{0, 0, stride}; }

enum { MK_PLAIN = 0, MK_HIDDEN = 1, MK_MODULATED = 2 };
struct MkOperand {
    int mode, swap, kfast, C;
    const float* p;            // PLAIN: the matrix.  HIDDEN: pe.  MODULATED: m
    MkIdx o, k;
    const float* w1; const float* b1;      // HIDDEN
    const float* x; const int* src;        // MODULATED
};
struct MkGemm {
    MkOperand a, b;
    i64 M, N, K;
    float* out; MkIdx om, on; const float* bias; int accumulate;
    float* part; int cps;      // slices > 1: partial tiles [slice][M][N]
};

__device__ __forceinline__ float mk_load(const MkOperand& op, i64 u, i64 k) {
    if (op.mode == MK_PLAIN) return op.p[mk_at(op.o, u) + mk_at(op.k, k)];
    const i64 r_ = op.swap ? k : u, c_ = op.swap ? u : k;
    if (op.mode == MK_HIDDEN) {
        const float* pe = op.p + r_ * 3;
        const float* w = op.w1 + c_ * 3;
        return mk_lrelu(((w[0] * pe[0] + w[1] * pe[1]) + w[2] * pe[2]) + op.b1[c_]);
    }
    const int j = (int)c_;                                           // (r_ is the pixel, c_ = j < 16 C)
    const int sp = op.src[r_ * 16 + j / op.C];
    if (sp < 0) return 0.f;
    return op.p[r_ * 16 * op.C + j] * op.x[(i64)sp * op.C + j % op.C];
}

template <bool MFMA>
__global__ __launch_bounds__(256) void mk_gemm_kernel(const MkGemm p) {
    constexpr int PITCH = MFMA ? 40 : 33;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 64 * PITCH * (MFMA ? 2 : 4)];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem);
    bf16_t* sb = sa + 64 * PITCH;
    float* fa = reinterpret_cast<float*>(smem);
    float* fb = fa + 64 * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kg = lane >> 5;
    const i64 ntn = (p.N + 63) / 64;
    const i64 m0 = ((i64)blockIdx.x / ntn) * 64, n0 = ((i64)blockIdx.x % ntn) * 64;
    const i64 nchunks = (p.K + 31) / 32;
    const i64 chunk0 = (i64)blockIdx.z * p.cps, chunk1 = chunk0 + p.cps < nchunks ? chunk0 + p.cps : nchunks;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ra[8], rb[8];
    auto fetch = [&](i64 chunk) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = e * 256 + tid;
            const int ua = p.a.kfast ? idx >> 5 : idx & 63, ka = p.a.kfast ? idx & 31 : idx >> 6;
            const int ub = p.b.kfast ? idx >> 5 : idx & 63, kb = p.b.kfast ? idx & 31 : idx >> 6;
            ra[e] = (m0 + ua < p.M && chunk * 32 + ka < p.K) ? mk_load(p.a, m0 + ua, chunk * 32 + ka) : 0.f;
            rb[e] = (n0 + ub < p.N && chunk * 32 + kb < p.K) ? mk_load(p.b, n0 + ub, chunk * 32 + kb) : 0.f;
        }
    };
    if (chunk0 < chunk1) fetch(chunk0);
    for (i64 chunk = chunk0; chunk < chunk1; ++chunk) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = e * 256 + tid;
            const int ua = p.a.kfast ? idx >> 5 : idx & 63, ka = p.a.kfast ? idx & 31 : idx >> 6;
            const int ub = p.b.kfast ? idx >> 5 : idx & 63, kb = p.b.kfast ? idx & 31 : idx >> 6;
            if constexpr (MFMA) {
                sa[ua * PITCH + ka] = rldm::f32_to_bf16(ra[e]);
                sb[ub * PITCH + kb] = rldm::f32_to_bf16(rb[e]);
            } else {
                fa[ua * PITCH + ka] = ra[e];
                fb[ub * PITCH + kb] = rb[e];
            }
        }
        __syncthreads();
        if (chunk + 1 < chunk1) fetch(chunk + 1);
        if constexpr (MFMA) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const uint4 a = *reinterpret_cast<const uint4*>(sa + (32 * (wave & 1) + l31) * PITCH + 16 * kk + 8 * kg);
                const uint4 bv = *reinterpret_cast<const uint4*>(sb + (32 * (wave >> 1) + l31) * PITCH + 16 * kk + 8 * kg);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
            }
        } else {
            for (int kk = 0; kk < 32; ++kk) {
                const float bv = fb[lane * PITCH + kk];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += fa[(16 * wave + r) * PITCH + kk] * bv;
            }
        }
    }
    // acc[r]: MFMA -> (m0 + 32 (wave & 1) + (r & 3) + 8 (r >> 2) + 4 kg, n0 + 32 (wave >> 1) + l31); fp32 -> (m0 + 16 wave + r, n0 + lane)
    const i64 n = MFMA ? n0 + 32 * (wave >> 1) + l31 : n0 + lane;
    if (n >= p.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const i64 m = MFMA ? m0 + 32 * (wave & 1) + (r & 3) + 8 * (r >> 2) + 4 * kg : m0 + 16 * wave + r;
        if (m >= p.M) continue;
        if (p.part) {
            p.part[((i64)blockIdx.z * p.M + m) * p.N + n] = acc[r];
        } else {
            float v = acc[r];
            if (p.bias) v += p.bias[n];
            float* o = p.out + mk_at(p.om, m) + mk_at(p.on, n);
            *o = p.accumulate ? *o + v : v;
        }
    }
}

// out (+)= (((0 + part[0]) + part[1]) + ...) (+ bias)
__global__ __launch_bounds__(256) void mk_reduce_kernel(const MkGemm p, int slices) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.M * p.N) return;
    float a = 0.f;
    for (int s = 0; s < slices; ++s) a += p.part[(i64)s * p.M * p.N + e];
    const i64 m = e / p.N, n = e % p.N;
    if (p.bias) a += p.bias[n];
    float* o = p.out + mk_at(p.om, m) + mk_at(p.on, n);
    *o = p.accumulate ? *o + a : a;
}

// ---- gathers and element-wise pieces of the backward -------------------------------------------------------------------------------
// Calls f(px, t) for every row (px, t) that reads input pixel (b, w, h), in a fixed order (i, wrapped copy of the column, j).
template <typename F>
__device__ __forceinline__ void mk_readers(const MkGeom& g, int b, int w, int h, F f) {
    for (int i = 0; i < 4; ++i) {
        const int hh = h + 1 - i;
        if (hh < 0 || hh % g.s) continue;
        const int ho = hh / g.s;
        if (ho >= g.Ho) continue;
        for (int q = w + 1 - g.W; q < g.W + 2; q += g.W) {            // the W + 2 wrapped columns that hold column w
            if (q < 0) continue;
            for (int j = 0; j < 4; ++j) {
                const int ww = q - j;
                if (ww < 0 || ww % g.s) continue;
                const int wo = ww / g.s;
                if (wo >= g.Wo) continue;
                f(((i64)b * g.Wo + wo) * g.Ho + ho, 4 * i + j);
            }
        }
    }
}

// dx[p][c] = sum over the rows that read p of G[row][c] m[row][c]
__global__ __launch_bounds__(256) void mk_dx_kernel(const MkGeom g, const float* __restrict__ G, const float* __restrict__ m,
                                                    float* __restrict__ dx) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= (i64)g.B * g.W * g.H * g.C) return;
    const int c = (int)(e % g.C);
    const i64 pix = e / g.C;
    const int h = (int)(pix % g.H), w = (int)((pix / g.H) % g.W), b = (int)(pix / ((i64)g.H * g.W));
    float a = 0.f;
    mk_readers(g, b, w, h, [&](i64 px, int t) {
        const i64 at = (px * 16 + t) * g.C + c;
        a += G[at] * m[at];
    });
    dx[e] = a;
}

// G[row][c] <- G[row][c] x[src[row]][c]
__global__ __launch_bounds__(256) void mk_dm_kernel(const float* __restrict__ x, const int* __restrict__ src, int C, i64 n, float* __restrict__ G) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int sp = src[e / C];
    G[e] = sp < 0 ? 0.f : G[e] * x[(i64)sp * C + e % C];
}

// dh[row][c] <- dh[row][c] lrelu'(pre[row][c])
__global__ __launch_bounds__(256) void mk_mask_kernel(const float* __restrict__ pe, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      int C, i64 n, float* __restrict__ dh) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float* q = pe + (e / C) * 3;
    const int c = (int)(e % C);
    const float pre = ((w1[c * 3] * q[0] + w1[c * 3 + 1] * q[1]) + w1[c * 3 + 2] * q[2]) + b1[c];
    dh[e] = dh[e] * mk_slope(pre);
}

// dr[p] = sum over the rows that read p as a tap of (dpe0 ci) ca + (dpe1 si) ca + dpe2 sa, minus the sixteen dpe0 of the pixel whose
// centre p is, plus that pixel's dr of the next layer
__global__ __launch_bounds__(256) void mk_dr_kernel(const MkGeom g, const float* __restrict__ dpe, const float* __restrict__ tab,
                                                    const float* __restrict__ dr_next, float* __restrict__ dr) {
    const i64 pix = (i64)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (i64)g.B * g.W * g.H) return;
    const int h = (int)(pix % g.H), w = (int)((pix / g.H) % g.W), b = (int)(pix / ((i64)g.H * g.W));
    float a = 0.f;
    mk_readers(g, b, w, h, [&](i64 px, int t) {
        const float* d = dpe + (px * 16 + t) * 3;
        a += ((d[0] * tab[32 + t]) * tab[t] + (d[1] * tab[48 + t]) * tab[t]) + d[2] * tab[16 + t];
    });
    if (w >= 1 && h >= 1 && (w - 1) % g.s == 0 && (h - 1) % g.s == 0 && (w - 1) / g.s < g.Wo && (h - 1) / g.s < g.Ho) {
        const i64 px = ((i64)b * g.Wo + (w - 1) / g.s) * g.Ho + (h - 1) / g.s;
        float c0 = 0.f;
        for (int t = 0; t < 16; ++t) c0 += dpe[(px * 16 + t) * 3];
        a -= c0;
        if (dr_next) a += dr_next[px];
    }
    dr[pix] = a;
}

__global__ __launch_bounds__(256) void mk_range_kernel(const float* __restrict__ x, i64 n, int C, float mean, float std_, float* __restrict__ r) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e < n) r[e] = (x[e * C] * std_ + mean) / 10.f;
}

__global__ __launch_bounds__(256) void mk_range_grad_kernel(const float* __restrict__ dr, i64 n, int C, float std_, float* __restrict__ dx) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dx[e * C] += (dr[e] / 10.f) * std_;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline bool mk_geom(const rldm_train_meta_desc* d, MkGeom* g) {
    if (!d || d->B < 1 || d->Win < 2 || d->Hin < 2 || (d->stride != 1 && d->stride != 2)) return false;
    if (!(d->C == 2 || (d->C > 0 && d->C % 16 == 0)) || !(d->N == 1 || (d->N > 0 && d->N % 16 == 0))) return false;
    *g = MkGeom{d->B, d->Win, d->Hin, d->C, d->N, d->stride, (d->Win - 2) / d->stride + 1, (d->Hin - 2) / d->stride + 1};
    // (pixel and row indices fit an int; element offsets are 64-bit)
    return (i64)d->B * d->Win * d->Hin < (1ll << 31) && (i64)d->B * g->Wo * g->Ho * 16 < (1ll << 31);
}

// K slices: enough workgroups to fill the device (2048), at least four 32-deep chunks per slice, at most 1024 slices (the gradients
// of the small matrices -- W1, and W2 of the narrow layers -- are one or a few tiles over millions of rows)
inline int mk_slices(i64 M, i64 N, i64 K, int* cps) {
    const i64 tiles = ((M + 63) / 64) * ((N + 63) / 64), nchunks = (K + 31) / 32;
    const i64 want = std::max<i64>(1, std::min<i64>({2048 / tiles, 1024, nchunks / 4}));
    *cps = (int)((nchunks + want - 1) / want);
    return (int)((nchunks + *cps - 1) / *cps);
}

inline i64 mk_part_bytes(i64 M, i64 N, i64 K) {
    int cps;
    const int s = mk_slices(M, N, K, &cps);
    return s > 1 ? (i64)s * M * N * (i64)sizeof(float) : 0;
}

inline int mk_gemm(MkGemm p, bool mfma, float* part, hipStream_t st) {
    int cps;
    const int slices = mk_slices(p.M, p.N, p.K, &cps);
    p.cps = cps;
    p.part = slices > 1 ? part : nullptr;
    const dim3 grid((unsigned)(((p.M + 63) / 64) * ((p.N + 63) / 64)), 1, (unsigned)slices);
    if (mfma) mk_gemm_kernel<true><<<grid, 256, 0, st>>>(p);
    else mk_gemm_kernel<false><<<grid, 256, 0, st>>>(p);
    if (slices > 1) mk_reduce_kernel<<<mk_nblk(p.M * p.N), 256, 0, st>>>(p, slices);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

inline MkOperand mk_plain(const float* p, MkIdx o, MkIdx k, int kfast) {
    return MkOperand{MK_PLAIN, 0, kfast, 0, p, o, k, nullptr, nullptr, nullptr, nullptr};
}
inline MkOperand mk_hidden(const float* pe, const float* w1, const float* b1, int swap) {
    return MkOperand{MK_HIDDEN, swap, swap ? 0 : 1, 0, pe, MkIdx{0, 0, 0}, MkIdx{0, 0, 0}, w1, b1, nullptr, nullptr};
}
inline MkOperand mk_modulated(const float* m, const float* x, const int* src, int C, int swap) {
    return MkOperand{MK_MODULATED, swap, swap ? 0 : 1, C, m, MkIdx{0, 0, 0}, MkIdx{0, 0, 0}, nullptr, nullptr, x, src};
}

struct MkSizes { i64 P, R, K; i64 g, dh, dpe, part; };
inline MkSizes mk_sizes(const MkGeom& g) {
    MkSizes s;
    s.P = (i64)g.B * g.Wo * g.Ho;
    s.R = s.P * 16;
    s.K = (i64)16 * g.C;
    s.g = s.R * g.C;
    s.dh = s.R * g.C;
    s.dpe = s.R * 3;
    s.part = std::max<i64>({mk_part_bytes(s.P, g.N, s.K), mk_part_bytes(s.P, s.K, g.N), mk_part_bytes(g.N, s.K, s.P), mk_part_bytes(s.R, g.C, g.C),
                            mk_part_bytes(g.C, g.C, s.R), mk_part_bytes(g.C, 3, s.R), mk_part_bytes(s.R, 3, g.C)}) / (i64)sizeof(float);
    return s;
}

}  // namespace

extern "C" {

int rldm_train_meta_ok(const rldm_train_meta_desc* d) {
    MkGeom g;
    return mk_geom(d, &g) ? 1 : 0;
}

int rldm_train_meta_range(const float* x, int64_t npix, int C, float range_mean, float range_std, float* r, void* stream) {
    RLDM_REQUIRE(x && r && npix >= 1 && C >= 1, "rldm_train_meta_range: null argument");
    mk_range_kernel<<<mk_nblk(npix), 256, 0, (hipStream_t)stream>>>(x, npix, C, range_mean, range_std, r);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_train_meta_range_grad(const float* dr, int64_t npix, int C, float range_std, float* dx, void* stream) {
    RLDM_REQUIRE(dr && dx && npix >= 1 && C >= 1, "rldm_train_meta_range_grad: null argument");
    mk_range_grad_kernel<<<mk_nblk(npix), 256, 0, (hipStream_t)stream>>>(dr, npix, C, range_std, dx);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t rldm_train_meta_workspace(const rldm_train_meta_desc* d) {
    MkGeom g;
    if (!mk_geom(d, &g)) return -1;
    const MkSizes s = mk_sizes(g);
    return (s.g + s.dh + s.dpe + s.part) * (int64_t)sizeof(float);
}

int rldm_train_meta_forward(const rldm_train_meta_desc* d, const float* x, const float* r, const float* tables, const float* w1,
                            const float* b1, const float* w2, const float* b2, const float* coov, const float* bias, float* y,
                            float* r_next, float* pe, int32_t* src, float* m, void* workspace, int64_t workspace_bytes, void* stream) {
    MkGeom g;
    RLDM_REQUIRE(mk_geom(d, &g), "rldm_train_meta_forward: no instance for this shape (C = 2 | 16 k, N = 1 | 16 k, stride 1 | 2, extents >= 2)");
    RLDM_REQUIRE(x && r && tables && w1 && b1 && w2 && b2 && coov && bias && y && pe && src && m, "rldm_train_meta_forward: null argument");
    RLDM_REQUIRE(workspace && workspace_bytes >= rldm_train_meta_workspace(d), "rldm_train_meta_forward: workspace smaller than rldm_train_meta_workspace");
    hipStream_t st = (hipStream_t)stream;
    const MkSizes s = mk_sizes(g);
    float* part = static_cast<float*>(workspace);
    mk_pe_kernel<<<mk_nblk(s.R), 256, 0, st>>>(g, r, tables, pe, src, r_next);
    RLDM_HIP_CHECK(hipGetLastError());
    // m[row][c] = sum_k h[row][k] W2[c][k] + b2[c]
    MkGemm q{mk_hidden(pe, w1, b1, 0), mk_plain(w2, mk_lin(g.C), mk_lin(1), 1), s.R, g.C, g.C, m, mk_lin(g.C), mk_lin(1), b2, 0, nullptr, 0};
    if (int e = mk_gemm(q, g.C >= 16, part, st)) return e;
    // y[px][n] = sum_j P[px][j] coov[n][(j % C) 16 + j / C] + bias[n]
    MkGemm c{mk_modulated(m, x, src, g.C, 0), mk_plain(coov, mk_lin(s.K), MkIdx{g.C, 1, 16}, 1), s.P, g.N, s.K, y, mk_lin(g.N), mk_lin(1),
             bias, 0, nullptr, 0};
    return mk_gemm(c, true, part, st);
}

int rldm_train_meta_backward(const rldm_train_meta_desc* d, const float* x, const float* dy, const float* tables, const float* w1,
                             const float* b1, const float* w2, const float* coov, const float* pe, const int32_t* src, const float* m,
                             const float* dr_next, float* dx, float* dr, float* dw1, float* db1, float* dw2, float* db2, float* dcoov,
                             float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
    MkGeom g;
    RLDM_REQUIRE(mk_geom(d, &g), "rldm_train_meta_backward: no instance for this shape");
    RLDM_REQUIRE(x && dy && tables && w1 && b1 && w2 && coov && pe && src && m, "rldm_train_meta_backward: null argument");
    const bool params = dw1 != nullptr;
    RLDM_REQUIRE(params ? (db1 && dw2 && db2 && dcoov && dbias) : (!db1 && !dw2 && !db2 && !dcoov && !dbias),
                 "rldm_train_meta_backward: the six parameter gradients come together or not at all");
    RLDM_REQUIRE(!dr || dx, "rldm_train_meta_backward: dr comes with dx");
    RLDM_REQUIRE(params || dx, "rldm_train_meta_backward: nothing to compute");
    RLDM_REQUIRE(workspace && workspace_bytes >= rldm_train_meta_workspace(d), "rldm_train_meta_backward: workspace smaller than rldm_train_meta_workspace");
    hipStream_t st = (hipStream_t)stream;
    const MkSizes s = mk_sizes(g);
    float* G = static_cast<float*>(workspace);
    float* dh = G + s.g;
    float* dpe = dh + s.dh;
    float* part = dpe + s.dpe;
    const bool mfma = g.C >= 16;
    // G[px][j] = sum_n dy[px][n] coov[n][(j % C) 16 + j / C]
    MkGemm q{mk_plain(dy, mk_lin(g.N), mk_lin(1), 1), mk_plain(coov, MkIdx{g.C, 1, 16}, mk_lin(s.K), 0), s.P, s.K, g.N, G, mk_lin(s.K),
             mk_lin(1), nullptr, 0, nullptr, 0};
    if (int e = mk_gemm(q, true, part, st)) return e;
    if (params) {
        // dcoov[n][(j % C) 16 + j / C] += sum_px dy[px][n] P[px][j]
        MkGemm c{mk_plain(dy, mk_lin(1), mk_lin(g.N), 0), mk_modulated(m, x, src, g.C, 1), g.N, s.K, s.P, dcoov, mk_lin(s.K),
                 MkIdx{g.C, 1, 16}, nullptr, 1, nullptr, 0};
        if (int e = mk_gemm(c, true, part, st)) return e;
        if (int e = rldm_train_colsum(dy, g.B, g.Wo * g.Ho, g.N, nullptr, 0, 0, dbias, stream)) return e;
    }
    if (dx) {
        mk_dx_kernel<<<mk_nblk((i64)g.B * g.W * g.H * g.C), 256, 0, st>>>(g, G, m, dx);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    mk_dm_kernel<<<mk_nblk(s.g), 256, 0, st>>>(x, src, g.C, s.g, G);          // G is dm from here on
    RLDM_HIP_CHECK(hipGetLastError());
    if (params) {
        // dW2[c][k] += sum_row dm[row][c] h[row][k]
        MkGemm c{mk_plain(G, mk_lin(1), mk_lin(g.C), 0), mk_hidden(pe, w1, b1, 1), g.C, g.C, s.R, dw2, mk_lin(g.C), mk_lin(1), nullptr, 1,
                 nullptr, 0};
        if (int e = mk_gemm(c, mfma, part, st)) return e;
        if (int e = rldm_train_colsum(G, g.B, g.Wo * g.Ho * 16, g.C, nullptr, 0, 0, db2, stream)) return e;
    }
    // dh[row][k] = sum_c dm[row][c] W2[c][k], then the LeakyReLU mask
    MkGemm hq{mk_plain(G, mk_lin(g.C), mk_lin(1), 1), mk_plain(w2, mk_lin(1), mk_lin(g.C), 0), s.R, g.C, g.C, dh, mk_lin(g.C), mk_lin(1),
              nullptr, 0, nullptr, 0};
    if (int e = mk_gemm(hq, mfma, part, st)) return e;
    mk_mask_kernel<<<mk_nblk(s.dh), 256, 0, st>>>(pe, w1, b1, g.C, s.dh, dh);
    RLDM_HIP_CHECK(hipGetLastError());
    if (params) {
        // dW1[k][e] += sum_row dpre[row][k] pe[row][e]  (fp32)
        MkGemm c{mk_plain(dh, mk_lin(1), mk_lin(g.C), 0), mk_plain(pe, mk_lin(1), mk_lin(3), 0), g.C, 3, s.R, dw1, mk_lin(3), mk_lin(1),
                 nullptr, 1, nullptr, 0};
        if (int e = mk_gemm(c, false, part, st)) return e;
        if (int e = rldm_train_colsum(dh, g.B, g.Wo * g.Ho * 16, g.C, nullptr, 0, 0, db1, stream)) return e;
    }
    if (dr) {
        // dpe[row][e] = sum_k dpre[row][k] W1[k][e]  (fp32)
        MkGemm c{mk_plain(dh, mk_lin(g.C), mk_lin(1), 1), mk_plain(w1, mk_lin(1), mk_lin(3), 0), s.R, 3, g.C, dpe, mk_lin(3), mk_lin(1),
                 nullptr, 0, nullptr, 0};
        if (int e = mk_gemm(c, false, part, st)) return e;
        mk_dr_kernel<<<mk_nblk((i64)g.B * g.W * g.H), 256, 0, st>>>(g, dpe, tables, dr_next, dr);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
