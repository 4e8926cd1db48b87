// train_common.h -- what the training translation units share: train.hip (switch, scratch, folds, element-wise ops, losses, optimizer,
// packers), train_conv.hip, train_wgrad.hip, train_norm.hip and train_disc.hip.  Device pieces first (inlined into each file's kernels),
// then the host-internal declarations with the file that defines each.  Nothing here is part of the C ABI (include/rangeldm_hip.h).
#pragma once
#include "common.h"
#include "../../include/rangeldm_hip.h"

namespace rldm::train {

// Four consecutive floats of a parameter or gradient view (bias, gamma, beta, dw ...).  The trainers pack these views end to end in flat
// buffers (tape.py: _init_parameters), so one starts at ANY 4-byte offset -- behind the VAE's 2-channel bias, 8 bytes off a 16-byte
// boundary -- and its alignment is 4 bytes.  The code says so: four element accesses, no cast to a 16-byte type.  (The compiler still
// merges them into one dwordx4 instruction, which global memory on this target takes at 4-byte alignment: same machine code, no claim.)
__device__ __forceinline__ f32x4 tr_load4(const float* __restrict__ p) { return f32x4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void tr_store4(float* __restrict__ p, const f32x4 v) { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }

// dw[n][c][t] += sum over slices of part[t][slice][n][c], four channels per thread (Cin % 4 == 0), `nb` workgroups of `nt` threads
// striding over the (tap, channel quad) items: the body of tr_wgrad_reduce_vec_kernel, also run as a rider of the next conv launch.
__device__ inline void tr_wgrad_reduce_items(const float* __restrict__ part, int slices, int N, int Cin, int taps, float* __restrict__ dw,
                                             int block, int nb, int nt) {
    const size_t nc = (size_t)N * Cin, nc4 = nc >> 2, items = nc4 * taps;
    for (size_t i = (size_t)block * nt + threadIdx.x; i < items; i += (size_t)nb * nt) {
        const int t = (int)(i / nc4);
        const size_t e = (i - (size_t)t * nc4) * 4;
        const float* src = part + (size_t)t * slices * nc + e;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int sidx = 0;
        for (; sidx + 8 <= slices; sidx += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(sidx + j) * nc);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        for (; sidx < slices; ++sidx) acc += *reinterpret_cast<const f32x4*>(src + (size_t)sidx * nc);
#pragma unroll
        for (int q = 0; q < 4; ++q) dw[(e + q) * taps + t] += acc[q];
    }
}

// source pixel of output pixel (b, wo, ho) under tap (dw, dh): index into the input's pixel array, or -1 for a zero.
// mode 0: plain; 1: nearest x2 (virtual input is twice as large); 2: zero insertion (virtual odd coordinates are zeros)
// shift: 0 for the symmetric pad; end-only padding (one wrapped column behind W, one zero row behind H) moves every tap by +1 in the
// stride-2 forward / weight gradient and by -1 in the zero-insertion data gradient (|shift| <= 1, so one wrap step still suffices)
__device__ inline int src_pixel(int b, int wo, int ho, int dw, int dh, int stride, int mode, int Win, int Hin, int shift) {
    const int sh = mode ? 1 : 0;
    const int Wv = Win << sh, Hv = Hin << sh;
    int vw = wo * stride + dw + shift, vh = ho * stride + dh + shift;
    if (vh < 0 || vh >= Hv) return -1;
    vw = vw < 0 ? vw + Wv : (vw >= Wv ? vw - Wv : vw);
    if (mode == 2 && ((vw | vh) & 1)) return -1;
    return (b * Win + (vw >> sh)) * Hin + (vh >> sh);
}

// 8 consecutive fp32 -> bf16x8; `valid` elements exist (the rest are zeros); vec: the row is 16-byte aligned
__device__ inline bf16x8 load_bf16x8_from_f32(const float* p, int valid, bool vec) {
    float f[8];
    if (vec && valid >= 8) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = e < valid ? p[e] : 0.f;
    }
    uint4 u;
    u.x = rldm::pack_bf16x2(f[0], f[1]); u.y = rldm::pack_bf16x2(f[2], f[3]);
    u.z = rldm::pack_bf16x2(f[4], f[5]); u.w = rldm::pack_bf16x2(f[6], f[7]);
    return __builtin_bit_cast(bf16x8, u);
}

// (round 5) what the fused launches fold into a conv / weight-gradient kernel (include/rangeldm_hip.h: rldm_train_fuse).  A tensor's
// GroupNorm statistics travel as per-(image, channel) (sum, sum of squares) pairs "cs" [B][C][2], accumulated by the epilogue of the
// conv that produced the tensor; a consumer derives (mean, rstd) of its groups from them (a concatenated input = two sources with their
// own pairs: groups may straddle the seam).  The GroupNorm backward sums travel the same way: "gs" [B][C][2] = (sum dz, sum dz xhat).
struct TrFuse {
    const float* x1; int C0;                       // second source of the input: channels [C0, Cin) (null: one source)
    const float* cs0; const float* cs1;            // input = act(GroupNorm(cat(x, x1))) built while staging (cs0 null: plain input)
    const float* gamma; const float* beta; int silu, groups; float eps;
    float* cs_out;                                 // += (sum, sumsq) of y per (image, channel)
    const float* g0; const float* g1; int G0;      // data-gradient epilogue: y = d act(GroupNorm(cat(g0, g1))) -> dz = y act'(z) stored,
    const float* gcs0; const float* gcs1;          //   gs_out += (sum dz, sum dz xhat)
    const float* ggamma; const float* gbeta; int gsilu, ggroups; float geps;
    float* gs_out;
    union {
        unsigned* tickets;                         // split-K launches: a zeroed arrival counter per output tile (left zeroed)
        float* part;                               // deterministic instances (never split): the tiles' partial rows [P / 64][N][2]
    };
    // a rider: the reduction of the PREVIOUS weight-gradient launch's partial tiles (it does not depend on this conv, and as a launch of
    // its own it cost ~10 us 47 times per step): run by extra z-planes of this launch's grid (rz0 = the first of them; rblocks = 0: none)
    const float* rpart; float* rdw; int rslices, rN, rCin, rtaps, rz0, rblocks;
};

// (deterministic mode) one fp32 operation, rounded on its own: a product never fuses with the sum it feeds, so a host restates the sums
__device__ __forceinline__ float det_add(const float a, const float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float det_mul(const float a, const float b) {
#pragma clang fp contract(off)
    return a * b;
}

// Two sigmoids, different arithmetic, both kept.  tr_sigmoid (v_exp_f32 + v_rcp_f32, ~1 ulp) is what the staging and tile-epilogue paths of
// the conv / weight-gradient kernels use: the IEEE division of 1.f / x costs ten more instructions per element of every staged tile.
// sigmoid_f (IEEE division) is what the stand-alone GroupNorm and SiLU kernels use.
__device__ inline float tr_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.f + __expf(-z)); }
__device__ inline float sigmoid_f(float z) { return 1.f / (1.f + __expf(-z)); }

// the fixed tree of every fp64 block sum: lanes l and l ^ 32, ^ 16 .. ^ 1, then the waves in order
__device__ inline double block_sum_d(double v, double* sh) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
    return t;
}

// ---- GroupNorm arithmetic, stated once ----------------------------------------------------------------------------------------------
// moments of a group from (sum, sum of squares, count) in fp64, the variance clamped at 0; then one of two finishes
struct GnMoments { double mean, var; };
__device__ __forceinline__ GnMoments gn_moments(const double s, const double ss, const double n) {
    const double mean = s / n;
    double var = ss / n - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    return {mean, var};
}
// fp64 1 / sqrt: the stand-alone statistics kernels (and the all-taps weight gradient's coefficients)
__device__ __forceinline__ float gn_rstd_f64(const double var, const float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }
// fp32 rsqrtf: the coefficients the fused convs build from "cs"
__device__ __forceinline__ float gn_rstd_f32(const double var, const float eps) { return rsqrtf((float)var + eps); }

// (s, ss) += the "cs" pairs of group g of image img over a two-source tensor (channels [0, C0) in cs0, the rest in cs1; see TrFuse)
__device__ __forceinline__ void gn_group_sum2(const float* cs0, const float* cs1, int C0, int C1, size_t img, int g, int cpg, double& s,
                                              double& ss) {
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        const float2 v = c < C0 ? reinterpret_cast<const float2*>(cs0)[img * C0 + c] : reinterpret_cast<const float2*>(cs1)[img * C1 + c - C0];
        s += (double)v.x; ss += (double)v.y;
    }
}

// backward element step: xh = (x - mean) rstd; z = xh gamma + beta; dz = dy act'(z)  (act = SiLU or the identity)
struct GnBwdElem { float xh, dz; };
__device__ __forceinline__ GnBwdElem gn_bwd_elem(float x, float dy, float mean, float rstd, float gamma, float beta, int silu) {
    const float xh = (x - mean) * rstd;
    float dz = dy;
    if (silu) {
        const float z = xh * gamma + beta, sg = sigmoid_f(z);
        dz *= sg * (1.f + z * (1.f - sg));
    }
    return {xh, dz};
}

// y = x * a + b = GroupNorm(x) for the channels [c_lo, c_hi) of image `img` of a (possibly two-source) tensor with npix pixels per
// image: sc[c] = (a, b).  Every thread sums its own channel's group from global memory (<= 24 pairs, L2 hits): no barrier inside, the
// caller synchronises before sc is read.
__device__ inline void tr_gn_coeffs(float2* sc, int c_lo, int c_hi, const float* cs0, const float* cs1, int C0, int C, int img, int groups,
                                    float eps, int npix, const float* gamma, const float* beta) {
    const int C1 = C - C0, cpg = C / groups;
    for (int ch = c_lo + (int)threadIdx.x; ch < c_hi; ch += blockDim.x) {
        double s = 0.0, ss = 0.0;
        gn_group_sum2(cs0, cs1, C0, C1, (size_t)img, ch / cpg, cpg, s, ss);
        const GnMoments m = gn_moments(s, ss, (double)npix * cpg);
        const float a = gn_rstd_f32(m.var, eps) * gamma[ch];
        sc[ch] = make_float2(a, beta[ch] - (float)m.mean * a);
    }
}

// the same for the BN channels [n0, n0 + BN) only, with (mean, rstd) kept: ce[cl] = (a, b, mean, rstd); every thread sums its own group
// from global memory (<= 24 pairs, L2 hits).  No barrier inside: the caller synchronises before ce is read.
__device__ inline void tr_gn_coeffs_tile(float4* ce, int BN, int n0, const float* cs0, const float* cs1, int C0, int C, int img, int groups,
                                         float eps, int npix, const float* gamma, const float* beta) {
    const int C1 = C - C0, cpg = C / groups;
    for (int cl = threadIdx.x; cl < BN; cl += blockDim.x) {
        const int ch = n0 + cl;
        if (ch >= C) { ce[cl] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
        double s = 0.0, ss = 0.0;
        gn_group_sum2(cs0, cs1, C0, C1, (size_t)img, ch / cpg, cpg, s, ss);
        const GnMoments m = gn_moments(s, ss, (double)npix * cpg);
        const float rstd = gn_rstd_f32(m.var, eps), a = rstd * gamma[ch];
        ce[cl] = make_float4(a, beta[ch] - (float)m.mean * a, (float)m.mean, rstd);
    }
}

// ---- host-internal --------------------------------------------------------------------------------------------------------------------
inline unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }
#define TR_LAUNCH_CHECK() RLDM_HIP_CHECK(hipGetLastError())

// train.hip: the deterministic switch (rldm_train_deterministic), read by every entry point when its launches are enqueued
bool deterministic();
// train.hip: the scratch buffers of the training library, one per slot, ONE owner.  -> *out: at least `bytes` of the slot's buffer;
// `zeroed`: a new block is zeroed once (tickets / accumulators, which every user leaves zeroed).  Growth rounds up to `min_bytes`.
enum TrScratchSlot { kFuseTickets, kGnAccumulators, kWgradPartials, kGroupPartials, kGroupTickets, kDetPartials, kScratchSlots };
int tr_scratch(TrScratchSlot slot, size_t bytes, size_t min_bytes, bool zeroed, hipStream_t st, void** out);
// (the partial rows of the deterministic mode's sums: written and folded by consecutive launches of one call)
inline int det_partials(size_t bytes, hipStream_t st, void** out) { return tr_scratch(kDetPartials, bytes, 1u << 20, false, st, out); }

// train.hip: launchers of its fold / zero kernels (each returns non-zero when the launch failed)
int launch_zero(float* y, size_t n, hipStream_t st);                 // tr_zero_kernel: a kernel, not a memset node
int launch_zero2d(float* y, int ld, int N, int B, hipStream_t st);   // tr_zero2d_kernel: y[b][0 .. N) = 0, rows ld apart
// tr_fold_rows_kernel (deterministic mode): out[o][i] (+)= part[o][0][i] + ... + part[o][nparts - 1][i], in that order
int launch_fold_rows(const float* part, int outer, int nparts, int inner, float* out, int out_ld, int accumulate, hipStream_t st);

// train.hip: K scalar fp64 sums out[0 .. K) over `nparts` blocks (every loss).  begin -> *dst: det: partial rows [K][nparts] (`partials`, or
// the library's own) for the kernel's <true> instance, else the zeroed `out` for the atomics of <false>.  end: det: the K folds.
int sums_begin(bool det, int K, unsigned nparts, double* out, double* partials, hipStream_t st, double** dst);
int sums_end(bool det, int K, unsigned nparts, const double* dst, double* out, hipStream_t st);

// train_wgrad.hip owns the pending-reduction rider (rldm_train_defer_reduce): flush_reduce launches it on its own; attach_reduce hands
// it to a conv launch of gx x gy workgroups per z-plane -> the extra z-planes (0: nothing pending or flushed instead; < 0: failed)
int flush_reduce();
int attach_reduce(TrFuse& f, hipStream_t st, unsigned gx, unsigned gy, unsigned gz);

// train_conv.hip: a desc's `mode` = the input transform (0, 1, 2) | RLDM_TRAIN_PAD_END.  -> *plain: the desc with the flag taken off
// (its symmetric twin: same shapes, same launch plan), *pad: 0 | 1.  false: "bad conv desc" -- an unknown mode, or end-only padding on
// anything but the 3x3 stride-2 forward / weight gradient (mode 0) and its zero-insertion data gradient (stride 1, mode 2).
bool conv_desc_split(const rldm_train_conv_desc* d, rldm_train_conv_desc* plain, int* pad);
inline int conv_desc_shift(const rldm_train_conv_desc* plain, int pad) { return !pad ? 0 : (plain->mode == 2 ? -1 : 1); }   // src_pixel's tap shift

inline TrFuse to_device_fuse(const rldm_train_fuse* fu, int Cin, int N) {
    TrFuse f{};
    if (!fu) { f.C0 = Cin; return f; }
    f.x1 = fu->x1; f.C0 = fu->x1 ? fu->C0 : Cin;
    f.cs0 = fu->cs0; f.cs1 = fu->cs1; f.gamma = fu->gamma; f.beta = fu->beta; f.silu = fu->silu; f.groups = fu->groups; f.eps = fu->eps;
    f.cs_out = fu->cs_out;
    f.g0 = fu->g0; f.g1 = fu->g1; f.G0 = fu->g1 ? fu->G0 : N; f.gcs0 = fu->gcs0; f.gcs1 = fu->gcs1; f.ggamma = fu->ggamma; f.gbeta = fu->gbeta;
    f.gsilu = fu->gsilu; f.ggroups = fu->ggroups; f.geps = fu->geps; f.gs_out = fu->gs_out;
    return f;
}

}  // namespace rldm::train
