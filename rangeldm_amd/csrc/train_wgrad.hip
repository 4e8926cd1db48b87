// train_wgrad.hip -- weight and bias gradients of the training step (rldm_train_wgrad*, rldm_train_colsum,
// rldm_train_linear_rows_wgrad).  dW[n][c][tap] = sum_p dy[p][n] * x[src(p, tap)][c]: pixels are the contraction index.
//   tr_wgrad_kernel         one tap per workgroup, any shape: every wave stores a partial tile, tr_wgrad_reduce_kernel adds them (no atomics).
//   tr_wgrad2_kernel        all taps per workgroup (stride 1, 64-multiples of channels, H a power of two <= 16: wgrad_v2_shape): partial
//                           tiles per K slice + tr_wgrad_reduce_vec_kernel, or (1x1, default mode) atomics straight into the gradient.
//   tr_wgrad2_group_kernel  the queue (rldm_train_wgrad_group): the all-taps gradients of many layers in one launch, the slices of a
//                           tile summed in slice order by the tile's last arriver.
//   the rider               rldm_train_defer_reduce: the last all-taps launch's reduction waits here (this file owns its state) for a conv
//                           launch to ride on (attach_reduce, called by train_conv.hip), or is flushed by whatever comes first.
//   tr_colsum*              bias / time-embedding-row gradients: per-image column sums of dy (fixed order in the deterministic mode).
#include "train_common.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace rldm::train;

namespace {

// ---- weight gradient --------------------------------------------------------------------------------------------------
struct TrWgrad {
    const float* dy; const float* x; float* dw;   // dw: partial sums [taps][slices][N][Cin], slices = grid.z * 4 waves
    int B, Win, Hin, Cin, Wout, Hout, N, taps, stride, mode, chunk, shift;   // chunk: pixels per wave (multiple of 16); shift: src_pixel
};

// 16 consecutive channels of one pixel row: `valid` of them exist; vec: the row pointer is 16-byte aligned
__device__ inline void load_row16(const float* p, int valid, bool vec, float* out) {
    if (vec && valid >= 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = reinterpret_cast<const float4*>(p)[q];
            out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) out[e] = e < valid ? p[e] : 0.f;
    }
}

// grid (n tiles * c tiles, taps, K splits), 4 waves: wave v contracts pixels [((z * 4 + v) * chunk), + chunk) for a 64 x 64
// tile of dW (2 x 2 MFMA tiles).  D[n][c] += A[n][k] B[k][c] with k = pixel, while memory has channels contiguous: every
// k-step the wave loads 16 pixel rows x 64 channels of dy and of x (tap-shifted) with coalesced 16-byte loads into its
// private LDS tile and reads the fragments back transposed (8 pixels of one channel per lane).
constexpr int WG_PITCH = 68;                     // floats: 16-byte aligned rows, conflict-free column reads
__global__ __launch_bounds__(256) void tr_wgrad_kernel(const TrWgrad p) {
    __shared__ __attribute__((aligned(16))) float sm[4][2][16][WG_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, kg = lane >> 5;
    const int ct = (p.Cin + 63) / 64;
    const int n0 = (blockIdx.x / ct) * 64, c0 = (blockIdx.x % ct) * 64;
    const int t = blockIdx.y;
    const int dw = p.taps == 9 ? t / 3 - 1 : 0, dh = p.taps == 9 ? t % 3 - 1 : 0;
    const int P = p.B * p.Wout * p.Hout;
    const int kbeg = (blockIdx.z * 4 + wave) * p.chunk;
    const int kend = min(kbeg + p.chunk, P);
    float (*sA)[WG_PITCH] = sm[wave][0];
    float (*sB)[WG_PITCH] = sm[wave][1];
    const int row = lane >> 2, seg = (lane & 3) * 16;          // staging role: pixel row of the k-step, 16-channel segment
    const bool vecA = (p.N & 3) == 0, vecB = (p.Cin & 3) == 0;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        const int px = k0 + row;
        float va[16], vb[16];
        int validA = 0, validB = 0;
        const float* pa = p.dy;
        const float* pb = p.x;
        if (px < kend) {
            validA = p.N - (n0 + seg);
            pa = p.dy + (size_t)px * p.N + n0 + seg;
            const int ho = px % p.Hout, t1 = px / p.Hout, wo = t1 % p.Wout, b = t1 / p.Wout;
            const int sp = src_pixel(b, wo, ho, dw, dh, p.stride, p.mode, p.Win, p.Hin, p.shift);
            if (sp >= 0) {
                validB = p.Cin - (c0 + seg);
                pb = p.x + (size_t)sp * p.Cin + c0 + seg;
            }
        }
        load_row16(pa, validA, vecA, va);
        load_row16(pb, validB, vecB, vb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<float4*>(&sA[row][seg + 4 * q]) = make_float4(va[4 * q], va[4 * q + 1], va[4 * q + 2], va[4 * q + 3]);
            *reinterpret_cast<float4*>(&sB[row][seg + 4 * q]) = make_float4(vb[4 * q], vb[4 * q + 1], vb[4 * q + 2], vb[4 * q + 3]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float a0[8], a1[8], b0[8], b1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a0[j] = sA[8 * kg + j][l31]; a1[j] = sA[8 * kg + j][32 + l31];
            b0[j] = sB[8 * kg + j][l31]; b1[j] = sB[8 * kg + j][32 + l31];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        auto pack8 = [](const float* f) {
            uint4 u;
            u.x = rldm::pack_bf16x2(f[0], f[1]); u.y = rldm::pack_bf16x2(f[2], f[3]);
            u.z = rldm::pack_bf16x2(f[4], f[5]); u.w = rldm::pack_bf16x2(f[6], f[7]);
            return __builtin_bit_cast(bf16x8, u);
        };
        const bf16x8 A0 = pack8(a0), A1 = pack8(a1), B0 = pack8(b0), B1 = pack8(b1);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B1, acc[1][1], 0, 0, 0);
    }
    // every wave stores its partial tile (coalesced along c); slices that had no pixels store zeros.
    // tile (i, j): lane (column c0 + 32 j + l31, half kg) holds rows n0 + 32 i + (r & 3) + 8 (r >> 2) + 4 kg
    const int slices = gridDim.z * 4, slice = blockIdx.z * 4 + wave;
    float* part = p.dw + ((size_t)t * slices + slice) * p.N * p.Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + 32 * j + l31;
            if (c >= p.Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = n0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kg;
                if (nn < p.N) part[(size_t)nn * p.Cin + c] = acc[i][j][r];
            }
        }
}

// Weight gradient, all taps in one workgroup (stride 1; every 3x3 / 1x1 conv of the UNet body).  The kernel above gives a
// workgroup ONE tap, so dy and x are read from L2 / HBM nine times per tile pair (604 MB for a 33 MB level-0 problem: it ran at
// the memory system's speed, 85 TFLOP/s).  Here a workgroup owns a 64 x 64 (n, c) tile for ALL taps over a range of pixel
// chunks.  A chunk = WC azimuth columns x all H beams of one image, staged once, transposed, as bf16:
//   sA[n][k]            k = h * WC + wl  (beam-major inside the chunk, so 8 consecutive k = 8 azimuth neighbours of a beam)
//   sB[d][c][(h + 1) * WC + wl] = x[w0 + wl + d - 1][h]   three copies pre-shifted by the azimuth tap (circular halo), beam
//                       rows -1 and H are zeros written once: the beam tap is a shift by WC elements = 16-byte aligned
// so every MFMA fragment of every tap is one aligned 16-byte LDS read: a wave does 9 MFMAs (one per tap, 32 x 32 x 16, its
// own quarter of the tile) per 10 fragment reads.  Staging lanes = 4 channel quads x 16 pixel pairs: 64-byte global segments
// and conflict-free 4-byte transposed LDS stores (pitch = odd number of 16-byte slots).  mode 1 (nearest x2 in front of the
// conv) is an index map at staging.  part: [taps][grid.y][N][Cin] partial sums (summed by tr_wgrad_reduce_kernel).
struct TrWgrad2 {
    const float* dy; const float* x; float* part;
    int B, W, H, Win, Hin, Cin, N, mode, lwc, cpw, nchunks, pitchA, pitchB;
    float* dw;                 // non-null: add the tile straight into the fp32 gradient [N][Cin][taps] (coalesced atomics), no partials
    float* rows; int rows_ld;  // bias / time-embedding-row gradients from the staged dy tile (workgroups of channel tile 0):
    float* total;              //   rows[b][n] += sum over image b's pixels, total[n] += sum over all pixels; either may be null
};

// (round 5) FU: x = act(GroupNorm(cat(x, x1))) rebuilt while staging (TrFuse's input side; the 64-channel tile lies in one source)
// (round 6) the kernel's body as a function of its place in the launch -- tile bx of the layer, K slice z of Z -- so that ONE launch can
// run the weight gradients of many layers (tr_wgrad2_group_kernel below).  GROUP: the slices of a tile meet through an arrival ticket
// and the LAST arriver sums the partial tiles in slice order into dw (deterministic; no reduction launch); Z == 1: the tile goes
// straight into dw.
// (round 6) V3: the staging rebuilt for images of 8 / 16 beams (the two high-resolution levels).  A LANE owns a channel of the tile and a
// wave every fourth 8-beam SEGMENT of the chunk: a wave-load is one 256-byte line, the contraction index runs beam-fastest
// (k = column * H + beam), so a segment is 16 contiguous bytes of its channel's LDS row (one ds_write_b128 instead of eight transposing
// ds_write_b32), GroupNorm + SiLU are applied once per element (the round-5 staging transformed every input element for each of its four
// azimuth-shifted roles) with the channel's coefficients in two registers, and the three copies a 3x3 needs are BEAM-shifted -- built
// from the segment's own ten registers -- while the azimuth taps are a shift by H elements (16-byte aligned for H >= 8) into a row
// staged with one halo column each side.  84 KB instead of 98 KB of fp32 per chunk and a fifth of the staging instructions -- and the
// grouped 3x3 launch of the two high-resolution levels takes 684 instead of 701 us (1x1: 174 / 180): what bounds these launches is not
// the staging but the L2-MISS TRAFFIC of fp32 activations (every (layer, slice) is read by (N / 64)(C / 64) tiles spread over the eight
// XCDs: 1.5 GB per launch at ~2.3 TB/s; profiles/round6_wgrad_ablation.txt).  bf16 activations would halve it; the tape stores fp32.
template <int TAPS, bool FU, bool GROUP, bool V3 = false>
__device__ __forceinline__ void tr_wgrad2_body(const TrWgrad2& p, const TrFuse& f, const int bx, const int z, const int Z, unsigned* tickets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
    constexpr int NC = TAPS == 9 ? 3 : 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kg = lane >> 5;
    const int WC = 1 << p.lwc, H = p.H, W = p.W, N = p.N, Cin = p.Cin;
    const int KP = WC * H;
    const int pitchA = p.pitchA, pitchB = V3 ? (WC + (TAPS == 9 ? 2 : 0)) * H + 8 : p.pitchB;
    bf16_t* sA = reinterpret_cast<bf16_t*>(wg_smem);                 // [64][pitchA]
    bf16_t* sB = sA + 64 * pitchA;                                   // [NC][64][pitchB]
    const int ct = Cin >> 6;
    const int n0 = (bx / ct) * 64, c0 = (bx % ct) * 64;
    const int wi = wave >> 1, wj = wave & 1;                         // this wave's 32 x 32 quarter of the tile
    if (TAPS == 9 && !V3) {                                          // zero beam rows -1 and H of the three copies
        for (int e = tid; e < NC * 64 * 2 * WC; e += 256) {
            const int wl = e & (WC - 1), r = (e >> p.lwc) & 1, rc = e >> (p.lwc + 1);
            sB[rc * pitchB + (r ? (H + 1) * WC : 0) + wl] = (bf16_t)0;
        }
    }
    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // staging role: 4 channel quads x 16 pixel pairs per wave (8 quads x 8 pairs = whole 128-byte lines measured the same)
    const int cq = 4 * wave + (lane & 3), ppl = lane >> 2;
    const int nwc = W >> p.lwc;
    const int sh = p.mode ? 1 : 0;
    struct WgStage { f32x4 d0, d1, xm, x0, x1, x2; };
    const float* const dyb = p.dy + n0 + 4 * cq;
    // (FU, two sources: the tile's 64 channels lie in one of them -- C0 % 64 == 0; xld = that source's channels per pixel)
    const bool second = FU && f.x1 != nullptr && c0 >= f.C0;
    const float* const xb = second ? f.x1 + (c0 - f.C0) + 4 * cq : p.x + c0 + 4 * cq;
    const int xld = FU ? (second ? Cin - f.C0 : f.C0) : Cin;
    const int Win = p.Win, Hin = p.Hin, lwc = p.lwc;
    // (FU) GroupNorm coefficients of the tile's channels for every image: sCo[b * 64 + c] = (a, b); after sB in the dynamic LDS
    float2* const sCo = reinterpret_cast<float2*>(sB + NC * 64 * pitchB);
    const bool in_gn = FU && f.cs0 != nullptr;
    if constexpr (FU) {
        if (in_gn) {
            const int cpg = Cin / f.groups, C1 = Cin - f.C0, npix = Win * Hin;
            for (int e = tid; e < p.B * 64; e += 256) {
                const int bi = e >> 6, ch = c0 + (e & 63);
                double s_ = 0.0, ss_ = 0.0;
                gn_group_sum2(f.cs0, f.cs1, f.C0, C1, (size_t)bi, ch / cpg, cpg, s_, ss_);
                const GnMoments m = gn_moments(s_, ss_, (double)npix * cpg);
                const float a = gn_rstd_f64(m.var, f.eps) * f.gamma[ch];
                sCo[e] = make_float2(a, f.beta[ch] - (float)m.mean * a);
            }
            // (visible after the first __syncthreads() of the chunk loop, before the first stash)
        }
    }
    auto fetch = [&](int pp, int b, int w0, WgStage& r) __attribute__((always_inline)) {
        const int k = 2 * pp, h = k >> lwc, wl = k & (WC - 1), hs = h >> sh;
        const float* src = dyb + ((size_t)(b * W + w0 + wl) * H + h) * N;
        r.d0 = *reinterpret_cast<const f32x4*>(src);
        r.d1 = *reinterpret_cast<const f32x4*>(src + (size_t)H * N);
        r.x0 = *reinterpret_cast<const f32x4*>(xb + ((size_t)(b * Win + ((w0 + wl) >> sh)) * Hin + hs) * xld);
        r.x1 = *reinterpret_cast<const f32x4*>(xb + ((size_t)(b * Win + ((w0 + wl + 1) >> sh)) * Hin + hs) * xld);
        if (TAPS == 9) {
            int wm = w0 + wl - 1, w2 = w0 + wl + 2;
            wm = wm < 0 ? wm + W : wm;
            w2 = w2 >= W ? w2 - W : w2;
            r.xm = *reinterpret_cast<const f32x4*>(xb + ((size_t)(b * Win + (wm >> sh)) * Hin + hs) * xld);
            r.x2 = *reinterpret_cast<const f32x4*>(xb + ((size_t)(b * Win + (w2 >> sh)) * Hin + hs) * xld);
        }
    };
    auto stash = [&](int pp, WgStage& r, int b) __attribute__((always_inline)) {
        const int k = 2 * pp, h = k >> lwc, wl = k & (WC - 1);
        if constexpr (FU) {
            if (in_gn) {
                const float2* co = sCo + b * 64 + 4 * cq;
                const bool act = f.silu != 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 cf = co[e];
                    float z0 = r.x0[e] * cf.x + cf.y, z1 = r.x1[e] * cf.x + cf.y;
                    if (act) { z0 *= tr_sigmoid(z0); z1 *= tr_sigmoid(z1); }
                    r.x0[e] = z0; r.x1[e] = z1;
                    if (TAPS == 9) {
                        float zm = r.xm[e] * cf.x + cf.y, z2 = r.x2[e] * cf.x + cf.y;
                        if (act) { zm *= tr_sigmoid(zm); z2 *= tr_sigmoid(z2); }
                        r.xm[e] = zm; r.x2[e] = z2;
                    }
                }
            }
        }
        uint32_t* da = reinterpret_cast<uint32_t*>(sA + (4 * cq) * pitchA + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) da[e * (pitchA >> 1)] = rldm::pack_bf16x2(r.d0[e], r.d1[e]);
        if (TAPS == 9) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(sB + (4 * cq) * pitchB + (h + 1) * WC + wl);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[e * (pitchB >> 1)] = rldm::pack_bf16x2(r.xm[e], r.x0[e]);
                dst[(64 + e) * (pitchB >> 1)] = rldm::pack_bf16x2(r.x0[e], r.x1[e]);
                dst[(128 + e) * (pitchB >> 1)] = rldm::pack_bf16x2(r.x1[e], r.x2[e]);
            }
        } else {
            uint32_t* dst = reinterpret_cast<uint32_t*>(sB + (4 * cq) * pitchB + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e * (pitchB >> 1)] = rldm::pack_bf16x2(r.x0[e], r.x1[e]);
        }
    };
    const int chunk_end = min((z + 1) * p.cpw, p.nchunks);
    const bool do_sums = (p.rows || p.total) && c0 == 0;
    int sum_b = -1;
    float sum_img = 0.f, sum_all = 0.f;
    if constexpr (!V3) {
    WgStage R[4];                                                    // one chunk of staging data (1 - 4 iterations of 6 loads)
    if (z * p.cpw < chunk_end) {
        const int c0_ = z * p.cpw, b0_ = c0_ / nwc, w00 = (c0_ - b0_ * nwc) << p.lwc;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (2 * (ppl + 16 * it) < KP) fetch(ppl + 16 * it, b0_, w00, R[it]);
    }
    for (int chunk = z * p.cpw; chunk < chunk_end; ++chunk) {
        const int b = chunk / nwc, w0 = (chunk - b * nwc) << p.lwc;
        __syncthreads();                                             // the previous chunk's fragments have been read
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (2 * (ppl + 16 * it) < KP) stash(ppl + 16 * it, R[it], b);
        __syncthreads();
        if (do_sums) {                                               // thread (row n = tid >> 2, quarter of the chunk's pixels)
            const bf16_t* r = sA + (tid >> 2) * pitchA + (tid & 3) * (KP >> 2);
            float sacc = 0.f;
            for (int k = 0; k < (KP >> 2); k += 2) {
                const uint32_t u = *reinterpret_cast<const uint32_t*>(r + k);
                sacc += rldm::bf16lo(u) + rldm::bf16hi(u);
            }
            sacc += __shfl_xor(sacc, 1);
            sacc += __shfl_xor(sacc, 2);
            if (b != sum_b) {
                if (sum_b >= 0 && p.rows && (tid & 3) == 0) unsafeAtomicAdd(p.rows + (size_t)sum_b * p.rows_ld + n0 + (tid >> 2), sum_img);
                sum_b = b;
                sum_img = 0.f;
            }
            sum_img += sacc;
            sum_all += sacc;
        }
        if (chunk + 1 < chunk_end) {                                 // the next chunk's loads fly during this chunk's MFMAs
            const int nb_ = (chunk + 1) / nwc, nw0 = ((chunk + 1) - nb_ * nwc) << p.lwc;
#pragma unroll
            for (int it = 0; it < 4; ++it)
                if (2 * (ppl + 16 * it) < KP) fetch(ppl + 16 * it, nb_, nw0, R[it]);
        }
        const bf16_t* fa = sA + (32 * wi + l31) * pitchA + 8 * kg;
        const bf16_t* fb = sB + (32 * wj + l31) * pitchB + 8 * kg;
        // fragments of k-step k + 1 are requested before the MFMAs of k-step k (one wave per SIMD: nothing else hides the LDS latency)
        if (TAPS == 9) {
            uint4 Ac = *reinterpret_cast<const uint4*>(fa), Bc[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) Bc[t] = *reinterpret_cast<const uint4*>(fb + (t / 3) * 64 * pitchB + (t % 3) * WC);
            for (int k = 0; k < KP; k += 16) {
                uint4 An = Ac, Bn[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) Bn[t] = Bc[t];
                if (k + 16 < KP) {
                    An = *reinterpret_cast<const uint4*>(fa + k + 16);
#pragma unroll
                    for (int t = 0; t < 9; ++t) Bn[t] = *reinterpret_cast<const uint4*>(fb + (t / 3) * 64 * pitchB + k + 16 + (t % 3) * WC);
                }
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, Ac), __builtin_bit_cast(bf16x8, Bc[t]), acc[t], 0, 0, 0);
                Ac = An;
#pragma unroll
                for (int t = 0; t < 9; ++t) Bc[t] = Bn[t];
            }
        } else {
#pragma unroll 2
            for (int k = 0; k < KP; k += 16) {
                const bf16x8 A = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + k));
                const bf16x8 Bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fb + k));
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, Bf, acc[0], 0, 0, 0);
            }
        }
    }
    } else {
        // ---- V3 staging (see the comment above the function) ----
        constexpr int HALO = TAPS == 9 ? 1 : 0, NE = TAPS == 9 ? 10 : 8;
        const int hsh = H == 16 ? 1 : 0, hmask = (1 << hsh) - 1;       // 8-beam segments per column: 1 << hsh
        const int nsx = (WC + 2 * HALO) << hsh, nsd = WC << hsh;         // segments of the (halo'd) input chunk / of dy (KP / 8 <= 16)
        const float* const dyc = p.dy + n0 + lane;
        const float* const xc = (second ? f.x1 + (c0 - f.C0) : p.x + c0) + lane;
        const size_t sN = (size_t)N, sX = (size_t)xld;
        float dv[4][8], xv[5][NE];
        auto fetch3 = [&](const int b, const int w0) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (a chunk of fewer than 16 segments -- 64 pixels -- : the surplus slots re-load the last segment and are not stored; a
                //  branch around the loads instead cost the common 16-segment case 20 %: 840 against 684 us for the grouped 3x3 launch)
                const int sg = min(wave + 4 * i, nsd - 1), wl = sg >> hsh, h0 = (sg & hmask) * 8;
                const float* src = dyc + ((size_t)(b * W + w0 + wl) * H + h0) * sN;
#pragma unroll
                for (int e = 0; e < 8; ++e) dv[i][e] = src[(size_t)e * sN];
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int sg = wave + 4 * i;
                if (sg < nsx) {
                    const int j = sg >> hsh, h0 = (sg & hmask) * 8;
                    int w = w0 + j - HALO;
                    w = w < 0 ? w + W : (w >= W ? w - W : w);
                    const float* src = xc + ((size_t)(b * W + w) * H + h0) * sX;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int h = h0 + e - HALO;
                        xv[i][e] = (h >= 0 && h < H) ? src[((ptrdiff_t)e - HALO) * (ptrdiff_t)sX] : 0.f;
                    }
                }
            }
        };
        auto stash3 = [&](const int b) __attribute__((always_inline)) {
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sg = wave + 4 * i;
                if (sg < nsd) {
                    u32x4 u;
                    u.x = rldm::pack_bf16x2(dv[i][0], dv[i][1]); u.y = rldm::pack_bf16x2(dv[i][2], dv[i][3]);
                    u.z = rldm::pack_bf16x2(dv[i][4], dv[i][5]); u.w = rldm::pack_bf16x2(dv[i][6], dv[i][7]);
                    *reinterpret_cast<u32x4*>(sA + lane * pitchA + 8 * sg) = u;
                }
            }
            float2 cf = make_float2(1.f, 0.f);
            if constexpr (FU) {
                if (in_gn) cf = sCo[b * 64 + lane];
            }
            const bool act = FU && in_gn && f.silu != 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int sg = wave + 4 * i;
                if (sg < nsx) {
                    const int h0 = (sg & hmask) * 8;
                    float v[NE];
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        float zz = xv[i][e];
                        if constexpr (FU) {
                            if (in_gn) {
                                zz = zz * cf.x + cf.y;
                                if (act) zz *= tr_sigmoid(zz);
                            }
                        }
                        v[e] = zz;
                    }
                    bf16_t* dst = sB + lane * pitchB + 8 * sg;
                    if constexpr (TAPS == 9) {
                        // (zero padding applies to the ACTIVATED tensor: the beams above / below the image)
                        if (h0 == 0) v[0] = 0.f;
                        if (h0 + 8 == H) v[9] = 0.f;
                        const unsigned p01 = rldm::pack_bf16x2(v[0], v[1]), p23 = rldm::pack_bf16x2(v[2], v[3]), p45 = rldm::pack_bf16x2(v[4], v[5]),
                                       p67 = rldm::pack_bf16x2(v[6], v[7]), p89 = rldm::pack_bf16x2(v[8], v[9]);
                        u32x4 m, lo, hi;                             // copies dh = 0 | -1 | +1: position h holds a[h + dh]
                        m.x = rldm::pack_bf16x2(v[1], v[2]); m.y = rldm::pack_bf16x2(v[3], v[4]); m.z = rldm::pack_bf16x2(v[5], v[6]); m.w = rldm::pack_bf16x2(v[7], v[8]);
                        lo.x = p01; lo.y = p23; lo.z = p45; lo.w = p67;
                        hi.x = p23; hi.y = p45; hi.z = p67; hi.w = p89;
                        *reinterpret_cast<u32x4*>(dst) = lo;
                        *reinterpret_cast<u32x4*>(dst + 64 * pitchB) = m;
                        *reinterpret_cast<u32x4*>(dst + 128 * pitchB) = hi;
                    } else {
                        u32x4 m;
                        m.x = rldm::pack_bf16x2(v[0], v[1]); m.y = rldm::pack_bf16x2(v[2], v[3]); m.z = rldm::pack_bf16x2(v[4], v[5]); m.w = rldm::pack_bf16x2(v[6], v[7]);
                        *reinterpret_cast<u32x4*>(dst) = m;
                    }
                }
            }
        };
        if (z * p.cpw < chunk_end) {
            const int c0_ = z * p.cpw, b0_ = c0_ / nwc, w00 = (c0_ - b0_ * nwc) << p.lwc;
            fetch3(b0_, w00);
        }
        for (int chunk = z * p.cpw; chunk < chunk_end; ++chunk) {
            const int b = chunk / nwc;
            __syncthreads();                                         // the previous chunk's fragments have been read
            stash3(b);
            __syncthreads();
            if (do_sums) {                                           // thread (row n = tid >> 2, quarter of the chunk's pixels)
                const bf16_t* r = sA + (tid >> 2) * pitchA + (tid & 3) * (KP >> 2);
                float sacc = 0.f;
                for (int k = 0; k < (KP >> 2); k += 2) {
                    const uint32_t u = *reinterpret_cast<const uint32_t*>(r + k);
                    sacc += rldm::bf16lo(u) + rldm::bf16hi(u);
                }
                sacc += __shfl_xor(sacc, 1);
                sacc += __shfl_xor(sacc, 2);
                if (b != sum_b) {
                    if (sum_b >= 0 && p.rows && (tid & 3) == 0) unsafeAtomicAdd(p.rows + (size_t)sum_b * p.rows_ld + n0 + (tid >> 2), sum_img);
                    sum_b = b;
                    sum_img = 0.f;
                }
                sum_img += sacc;
                sum_all += sacc;
            }
            if (chunk + 1 < chunk_end) {                             // the next chunk's loads fly during this chunk's MFMAs
                const int nb_ = (chunk + 1) / nwc, nw0 = ((chunk + 1) - nb_ * nwc) << p.lwc;
                fetch3(nb_, nw0);
            }
            const bf16_t* fa = sA + (32 * wi + l31) * pitchA + 8 * kg;
            const bf16_t* fb = sB + (32 * wj + l31) * pitchB + 8 * kg;
            if (TAPS == 9) {
                // tap t = (dw + 1) * 3 + (dh + 1): copy t % 3 (beam shift), t / 3 columns of H elements into the halo'd row
                uint4 Ac = *reinterpret_cast<const uint4*>(fa), Bc[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) Bc[t] = *reinterpret_cast<const uint4*>(fb + (t % 3) * 64 * pitchB + (t / 3) * H);
                for (int k = 0; k < KP; k += 16) {
                    uint4 An = Ac, Bn[9];
#pragma unroll
                    for (int t = 0; t < 9; ++t) Bn[t] = Bc[t];
                    if (k + 16 < KP) {
                        An = *reinterpret_cast<const uint4*>(fa + k + 16);
#pragma unroll
                        for (int t = 0; t < 9; ++t) Bn[t] = *reinterpret_cast<const uint4*>(fb + (t % 3) * 64 * pitchB + k + 16 + (t / 3) * H);
                    }
#pragma unroll
                    for (int t = 0; t < 9; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, Ac), __builtin_bit_cast(bf16x8, Bc[t]), acc[t], 0, 0, 0);
                    Ac = An;
#pragma unroll
                    for (int t = 0; t < 9; ++t) Bc[t] = Bn[t];
                }
            } else {
#pragma unroll 2
                for (int k = 0; k < KP; k += 16) {
                    const bf16x8 A = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + k));
                    const bf16x8 Bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fb + k));
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, Bf, acc[0], 0, 0, 0);
                }
            }
        }
    }
    if (do_sums && (tid & 3) == 0) {
        if (sum_b >= 0 && p.rows) unsafeAtomicAdd(p.rows + (size_t)sum_b * p.rows_ld + n0 + (tid >> 2), sum_img);
        if (p.total) unsafeAtomicAdd(p.total + n0 + (tid >> 2), sum_all);
    }
    // lane (column c = c0 + 32 wj + l31, half kg), register r <-> row n0 + 32 wi + (r & 3) + 8 (r >> 2) + 4 kg
    if (GROUP ? Z == 1 : p.dw != nullptr) {
        // the tile in the gradient's own layout ([n][c][tap]: 64 * TAPS contiguous floats per row) through LDS, 32 rows at a
        // time, then along a row: one cache line per 32 lanes (atomics; GROUP with one slice: this workgroup is the tile's only writer)
        constexpr int TP = 64 * TAPS + 1;
        float* tile = reinterpret_cast<float*>(wg_smem);
        for (int half = 0; half < 2; ++half) {
            __syncthreads();
            if (wi == half) {
#pragma unroll
                for (int t = 0; t < TAPS; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * kg) * TP + (32 * wj + l31) * TAPS + t] = acc[t][r];
            }
            __syncthreads();
            for (int e = tid; e < 32 * 64 * TAPS; e += 256) {
                const int row = e / (64 * TAPS), col = e - row * (64 * TAPS);
                float* dst = p.dw + ((size_t)(n0 + 32 * half + row) * Cin + c0) * TAPS + col;
                if (GROUP) *dst += tile[row * TP + col];
                else unsafeAtomicAdd(dst, tile[row * TP + col]);
            }
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
        float* part = p.part + (((size_t)t * Z + z) * N + n0 + 32 * wi + 4 * kg) * Cin + c0 + 32 * wj + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[(size_t)((r & 3) + 8 * (r >> 2)) * Cin] = acc[t][r];
    }
    if constexpr (GROUP) {
        // the tile's Z slices meet here: every workgroup publishes its partial tile (release at agent scope: the stores are written back
        // past this XCD's L2) and takes a ticket; the last one invalidates its caches (acquire) and sums the Z partial tiles in slice
        // order -- the same order whatever the arrival order, so the gradient is bit-reproducible -- into dw, and re-arms the ticket.
        __shared__ unsigned s_last;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (tid == 0) {
            const unsigned old = __hip_atomic_fetch_add(tickets + bx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = old == (unsigned)(Z - 1) ? 1u : 0u;
            if (s_last) __hip_atomic_store(tickets + bx, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!s_last) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // 16 columns x 16 rows per pass (a thread = one (row, column quad): 16-byte loads along c), slices in flight eight at a time
        const size_t nc = (size_t)N * Cin;
        const int cq4 = (tid & 15) * 4, rr = tid >> 4;
        for (int t = 0; t < TAPS; ++t)
            for (int r0 = 0; r0 < 64; r0 += 16) {
                const size_t e = (size_t)(n0 + r0 + rr) * Cin + c0 + cq4;
                const float* src = p.part + (size_t)t * Z * nc + e;
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                int sidx = 0;
                for (; sidx + 8 <= Z; sidx += 8) {
                    f32x4 v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(sidx + j) * nc);
#pragma unroll
                    for (int j = 0; j < 8; ++j) a += v[j];
                }
                for (; sidx < Z; ++sidx) a += *reinterpret_cast<const f32x4*>(src + (size_t)sidx * nc);
#pragma unroll
                for (int q = 0; q < 4; ++q) p.dw[(e + q) * TAPS + t] += a[q];
            }
    }
}

template <int TAPS, bool FU = false>
__global__ __launch_bounds__(256) void tr_wgrad2_kernel(const TrWgrad2 p, const TrFuse f) {
    tr_wgrad2_body<TAPS, FU, false>(p, f, blockIdx.x, blockIdx.y, gridDim.y, nullptr);
}

// ---- (round 6) the weight gradients of MANY layers in one launch --------------------------------------------------------------------
// A weight gradient depends on nothing that comes after it in backward, and nothing in backward depends on it: launched where the tape
// reaches them, the ~85 all-taps launches of a step each ran alone on the chip at its launch + first-touch + drain floor (1.8 ms of a
// 9.3 ms step for 0.27 TFLOP).  The host queues them instead (rldm_train_wgrad_group) and hands the queue to this kernel in groups of
// up to kWgGroupMax layers of one instantiation (the kernel-argument block holds the records: capture-safe, no descriptor upload):
// block id -> (layer, tile, K slice).
constexpr int kWgGroupMax = 22;
struct WgItem {
    const float* dy; const float* x; const float* x1; float* dw; float* rows; float* total; float* part;
    const float* cs0; const float* cs1; const float* gamma; const float* beta;
    int B, W, H, Win, Hin, Cin, N, mode, lwc, cpw, nchunks, Z, rows_ld, C0, silu, groups;
    float eps;
    unsigned ticket_off;
};
struct WgGroup {
    int n;
    unsigned* tickets;
    int first[kWgGroupMax + 1];         // first block of layer i (first[n] = the grid)
    WgItem item[kWgGroupMax];
};
static_assert(sizeof(WgGroup) <= 4096, "the group record is the kernel's argument block");

template <int TAPS, bool FU, bool V3>
__global__ __launch_bounds__(256) void tr_wgrad2_group_kernel(const WgGroup g) {
    const int bid = blockIdx.x;
    int l = 0;
    for (int i = 1; i < g.n; ++i) l = bid >= g.first[i] ? i : l;
    const WgItem& it = g.item[l];
    TrWgrad2 p;
    p.dy = it.dy; p.x = it.x; p.part = it.part; p.dw = it.dw; p.rows = it.rows; p.rows_ld = it.rows_ld; p.total = it.total;
    p.B = it.B; p.W = it.W; p.H = it.H; p.Win = it.Win; p.Hin = it.Hin; p.Cin = it.Cin; p.N = it.N; p.mode = it.mode; p.lwc = it.lwc;
    p.cpw = it.cpw; p.nchunks = it.nchunks;
    p.pitchA = (it.H << it.lwc) + 8;
    p.pitchB = ((TAPS == 9 ? it.H + 2 : it.H) << it.lwc) + 8;
    TrFuse f;
    f.x1 = it.x1; f.C0 = it.C0; f.cs0 = it.cs0; f.cs1 = it.cs1; f.gamma = it.gamma; f.beta = it.beta; f.silu = it.silu;
    f.groups = it.groups; f.eps = it.eps;
    // block -> (K slice, tile): tile fastest.  (Measured and dropped: a layout [Z / 8][tile][8] that puts the tiles of a slice -- which
    // read the same pixels of dy and x -- on one XCD behind one L2: 873 against 780 us for the 3x3 launch of the two high-resolution
    // levels, and the one-slice layers of the low levels, each on a single XCD, 529 against 307 us.  The kernel is bound by its staging
    // pipeline per CU -- one chunk of loads in flight, a transposing LDS write, two barriers per chunk -- not by L2 misses.)
    const int local = bid - g.first[l];
    const int tiles = (it.N >> 6) * (it.Cin >> 6);
    tr_wgrad2_body<TAPS, FU, true, V3>(p, f, local % tiles, local / tiles, it.Z, g.tickets + it.ticket_off);
}

// four channels per thread, eight slices in flight (Cin % 4 == 0): the scalar kernel below ran at 2 TB/s over 38 MB of partials
__global__ __launch_bounds__(256) void tr_wgrad_reduce_vec_kernel(const float* __restrict__ part, int slices, int N, int Cin, int taps,
                                                                  float* __restrict__ dw) {
    tr_wgrad_reduce_items(part, slices, N, Cin, taps, dw, blockIdx.x, gridDim.x, 256);
}

// dw[n][c][t] += sum over slices of part[t][slice][n][c]   (one thread per (t, n, c); reads coalesced along c)
__global__ __launch_bounds__(256) void tr_wgrad_reduce_kernel(const float* __restrict__ part, int slices, int N, int Cin, int taps,
                                                              float* __restrict__ dw) {
    const size_t nc = (size_t)N * Cin;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc * taps) return;
    const int t = (int)(i / nc);
    const size_t e = i % nc;
    const float* src = part + (size_t)t * slices * nc + e;
    float acc = 0.f;
    for (int s = 0; s < slices; ++s) acc += src[(size_t)s * nc];
    dw[e * taps + t] += acc;
}

// rows[b][n] += sum over the pixels of image b of dy[p][n]; total[n] += the same over all images.  grid (64-channel tiles,
// images, 256-pixel slabs), 256 threads = 16 pixel lanes x 16 channel quads (16-byte loads when N % 4 == 0): fp32 atomics
// into buffers the caller zeroed (rows) / accumulates into (total = bias gradient).
// DET (rldm_train_deterministic): the slab's sums are stored as a partial row instead -- rows = part [B][slabs][N] -- and
// tr_colsum_finish_kernel adds the slabs of an image, then the images, in index order.
template <bool DET = false>
__global__ __launch_bounds__(256) void tr_colsum_kernel(const float* __restrict__ dy, int npix, int N, float* __restrict__ rows,
                                                        int rows_ld, float* __restrict__ total) {
    __shared__ float sh[16][68];
    const int b = blockIdx.y, cq = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int ch = blockIdx.x * 64 + cq * 4;
    const int p0 = blockIdx.z * 256, p1 = min(p0 + 256, npix);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const float* base = dy + (size_t)b * npix * N + ch;
    if ((N & 3) == 0 && ch + 3 < N) {
        for (int px = p0 + pl; px < p1; px += 16) {
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)px * N);
            a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
        }
    } else {
        for (int px = p0 + pl; px < p1; px += 16) {
            const float* r = base + (size_t)px * N;
            if (ch < N) a0 += r[0];
            if (ch + 1 < N) a1 += r[1];
            if (ch + 2 < N) a2 += r[2];
            if (ch + 3 < N) a3 += r[3];
        }
    }
    sh[pl][cq * 4] = a0; sh[pl][cq * 4 + 1] = a1; sh[pl][cq * 4 + 2] = a2; sh[pl][cq * 4 + 3] = a3;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        if (c < N) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) v += sh[r][threadIdx.x];
            if constexpr (DET) rows[((size_t)b * gridDim.z + blockIdx.z) * N + c] = v;
            else {
                if (rows) unsafeAtomicAdd(rows + (size_t)b * rows_ld + c, v);
                if (total) unsafeAtomicAdd(total + c, v);
            }
        }
    }
}

// (deterministic mode) image sums = the slabs of part [B][S][N] added in slab order; rows[b][c] (+)= image sum; total[c] += the image
// sums added in image order.  One thread per channel.
__global__ __launch_bounds__(256) void tr_colsum_finish_kernel(const float* __restrict__ part, int B, int S, int N, float* __restrict__ rows,
                                                               int rows_ld, int rows_accumulate, float* __restrict__ total) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    float t = 0.f;
    for (int b = 0; b < B; ++b) {
        float a = 0.f;
        for (int z = 0; z < S; ++z) a = det_add(a, part[((size_t)b * S + z) * N + c]);
        if (rows) {
            float* d = rows + (size_t)b * rows_ld + c;
            *d = rows_accumulate ? det_add(*d, a) : a;
        }
        t = det_add(t, a);
    }
    if (total) total[c] = det_add(total[c], t);
}

// dw[n][k] += sum_b dy[b][n] x[b][k] (fp32 master gradient, row-major [N][K]); dbias[n] += sum_b dy[b][n]
__global__ __launch_bounds__(256) void tr_linear_rows_wgrad_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x,
                                                                   int ldx, int B, int N, int K, float* __restrict__ dw,
                                                                   float* __restrict__ dbias) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int kq = K >> 2;
    if (i >= (size_t)N * kq) return;
    const int n = (int)(i / kq), k = (int)(i % kq) * 4;
    f32x4 acc = tr_load4(dw + (size_t)n * K + k);
    float sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = dy[(size_t)b * ldy + n];
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)b * ldx + k);
        acc += g * xv;
        sb += g;
    }
    tr_store4(dw + (size_t)n * K + k, acc);
    if (k == 0 && dbias) dbias[n] += sb;
}

// The reduction of the last all-taps weight-gradient launch's partial tiles, waiting for a conv launch to ride on
// (rldm_train_defer_reduce; one caller thread, stream ordered).
struct PendingReduce { const float* part = nullptr; float* dw = nullptr; int slices = 0, N = 0, Cin = 0, taps = 0; hipStream_t st = nullptr; };
PendingReduce g_red;
int g_defer_reduce = 0;

}  // namespace

int rldm::train::flush_reduce() {
    if (!g_red.part) return 0;
    tr_wgrad_reduce_vec_kernel<<<nblk((size_t)g_red.N * g_red.Cin * g_red.taps / 4), 256, 0, g_red.st>>>(g_red.part, g_red.slices, g_red.N,
                                                                                                      g_red.Cin, g_red.taps, g_red.dw);
    g_red.part = nullptr;
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// attach the pending reduction to a conv launch of gx x gy workgroups per z-plane: -> extra z-planes
int rldm::train::attach_reduce(TrFuse& f, hipStream_t st, unsigned gx, unsigned gy, unsigned gz) {
    if (!g_red.part) return 0;
    if (g_red.st != st) { if (flush_reduce()) return -1; return 0; }
    const size_t items = (size_t)g_red.N * g_red.Cin * g_red.taps / 4;
    const int want = (int)std::min<size_t>((items + 255) / 256, 512);
    const int planes = (int)((want + (size_t)gx * gy - 1) / ((size_t)gx * gy));
    if (gz + planes > 65535) { if (flush_reduce()) return -1; return 0; }
    f.rpart = g_red.part; f.rdw = g_red.dw; f.rslices = g_red.slices; f.rN = g_red.N; f.rCin = g_red.Cin; f.rtaps = g_red.taps;
    f.rz0 = (int)gz; f.rblocks = want;
    g_red.part = nullptr;
    return planes;
}

// The shape rule of the all-taps kernels (tr_wgrad2_kernel): stride 1, 64-multiples of channels, H a power of two <= 16, and a chunk of
// WC = 1 << lwc azimuth columns that fits the LDS tiles and divides W.  -> lwc, or -1: the one-tap kernel.
static int wgrad_v2_shape(const rldm_train_conv_desc* d) {
    if (d->mode < 0 || d->mode > 2) return -1;          // (RLDM_TRAIN_PAD_END: the one-tap kernel)
    const int sh = d->mode ? 1 : 0;
    const int Wout = (d->Win << sh) / d->stride, Hout = (d->Hin << sh) / d->stride;
    if (!(d->stride == 1 && d->mode <= 1 && d->N % 64 == 0 && d->Cin % 64 == 0 && Hout >= 2 && Hout <= 16 && (Hout & (Hout - 1)) == 0)) return -1;
    for (int l = 6; l >= 3; --l)
        if ((Hout << l) <= 128 && ((Hout + 2) << l) <= 160 && Wout % (1 << l) == 0) return l;
    return -1;
}

// dynamic LDS of a tr_wgrad2 launch: sA [64][pitchA] + sB [3 | 1][64][pitchB] bf16 (V3 stages its own halo'd rows: tr_wgrad2_body),
// (fused) the tile's GroupNorm coefficients per image, and room for the fp32 tile where it goes through LDS straight into dw
static size_t wgrad2_lds_bytes(int taps, int H, int lwc, int pitchA, int pitchB, bool fused, int B, bool v3, bool into_dw) {
    if (v3) pitchB = ((1 << lwc) + (taps == 9 ? 2 : 0)) * H + 8;
    size_t smem = (size_t)64 * pitchA * 2 + (size_t)(taps == 9 ? 3 : 1) * 64 * pitchB * 2;
    if (fused) smem += (size_t)B * 64 * sizeof(float2);
    if (into_dw) smem = std::max(smem, (size_t)32 * (64 * taps + 1) * sizeof(float));
    return smem;
}

// the opt-in to more than 64 KiB of dynamic LDS, once per kernel table: 160 KiB for the direct kernels, 128 KiB for the grouped ones (which
// also have a static LDS word), as they were written; nobody recorded why the two differ, and the tiles need <= 88 KiB.
template <typename Kernel, size_t n>
static int wgrad2_allow_lds(Kernel* const (&kernels)[n], int bytes, bool* done) {
    for (size_t k = 0; k < n && !*done; ++k)
        RLDM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[k]), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    *done = true;
    return 0;
}

extern "C" {

int rldm_train_defer_reduce(int on) {
    g_defer_reduce = on;
    return on ? 0 : flush_reduce();
}

int rldm_train_flush_reduce(void) { return flush_reduce(); }

int rldm_train_reduce_pending(void) { return g_red.part ? 1 : 0; }

int rldm_train_wgrad_fused_ok(const rldm_train_conv_desc* d, const rldm_train_fuse* fu) {
    if (!d || !fu) return 0;
    if (wgrad_v2_shape(d) < 0 || d->mode != 0 || d->B > 16) return 0;
    if (fu->x1 && (fu->C0 <= 0 || fu->C0 >= d->Cin || fu->C0 % 64 != 0)) return 0;
    if (fu->cs0 && (fu->groups < 1 || d->Cin % fu->groups != 0 || !fu->gamma || !fu->beta || (fu->x1 && !fu->cs1))) return 0;
    return 1;
}

// ---- (round 6) grouped weight gradients: the queue ------------------------------------------------------------------------------------
// rldm_train_wgrad_group(1): all-taps weight gradients are queued instead of launched; rldm_train_wgrad_group_flush (or group(0)) runs
// the queue as a few launches of tr_wgrad2_group_kernel.  One caller thread, one stream per queue (a call on another stream flushes
// first, and so does queueing a dw that is already queued: two items of one launch must not add into the same dw); the caller keeps every
// queued operand alive and unmodified until the flush (rangeldm_amd/training.py does).  A flush empties the queue, failed or not.
struct WgQueued { WgItem it; int taps; bool fu, v3; int tiles; size_t part_floats; size_t smem; double unit; };
static std::vector<WgQueued> g_wgq;
static hipStream_t g_wgq_stream = nullptr;
static int g_wg_group = 0;

static int wg_group_launch() {
    hipStream_t st = g_wgq_stream;
    // K slices.  With every layer of a class in one launch the chip is full whatever a single layer brings, so the slices per tile --
    // partial tiles to write and re-read, a last arriver to sum them -- shrink from the launch-per-layer form's 64 to <= 16: a workgroup
    // takes `budget` units of work (a unit = a chunk of 128 pixels x 9 taps; a 1x1 tap set costs about a third).  Measured per class at
    // the RangeLDM size, batch 8 (profiles/round6_wgrad_group_budget.txt): 3x3 launches are fastest at 32 units (712 / 276 us; 16: 769 /
    // 307, 8: 996 / 434, 4: 1543 / 514 -- the last arriver's serial sum over the slices is the tail), the 1x1 launches at 8 - 16.
    for (auto& q : g_wgq) {
        const double budget = q.taps == 9 ? 32.0 : 12.0;
        WgItem& it = q.it;
        int cpw = std::max(1, (int)(budget / q.unit + 0.5));
        cpw = std::min(cpw, it.nchunks);
        int Z = (it.nchunks + cpw - 1) / cpw;
        cpw = (it.nchunks + Z - 1) / Z;
        Z = (it.nchunks + cpw - 1) / cpw;
        it.cpw = cpw; it.Z = Z;
        q.part_floats = Z > 1 ? (size_t)q.taps * Z * it.N * it.Cin : 0;
    }
    // scratch of the partial tiles (layers with more than one K slice) and the arrival tickets (every launch leaves them zeroed)
    size_t need = 0, ntick = 0;
    for (auto& q : g_wgq) { need += q.part_floats; ntick += (size_t)q.tiles; }
    float* scratch = nullptr;
    unsigned* tickets = nullptr;
    if (tr_scratch(kGroupPartials, need * sizeof(float), 0, false, st, reinterpret_cast<void**>(&scratch))) return 1;
    if (tr_scratch(kGroupTickets, ntick * sizeof(unsigned), 4096 * sizeof(unsigned), true, st, reinterpret_cast<void**>(&tickets))) return 1;
    typedef void (*GroupKernel)(const WgGroup);
    static const GroupKernel kernels[8] = {tr_wgrad2_group_kernel<9, false, false>, tr_wgrad2_group_kernel<1, false, false>,
                                           tr_wgrad2_group_kernel<9, true, false>,  tr_wgrad2_group_kernel<1, true, false>,
                                           tr_wgrad2_group_kernel<9, false, true>,  tr_wgrad2_group_kernel<1, false, true>,
                                           tr_wgrad2_group_kernel<9, true, true>,   tr_wgrad2_group_kernel<1, true, true>};
    static bool attr = false;
    if (wgrad2_allow_lds(kernels, 128 * 1024, &attr)) return 1;
    size_t poff = 0, toff = 0;
    for (auto& q : g_wgq) {
        q.it.part = scratch + poff; poff += q.part_floats;
        q.it.ticket_off = (unsigned)toff; toff += (size_t)q.tiles;
    }
    // one launch per (instantiation, <= kWgGroupMax layers), long workgroups first (the layers with the most pixels per slice)
    for (int cls = 0; cls < 8; ++cls) {
        const int taps = (cls & 1) ? 1 : 9;
        const bool fu = (cls & 2) != 0, v3 = (cls & 4) != 0;
        std::vector<const WgQueued*> sel;
        for (auto& q : g_wgq) if (q.taps == taps && q.fu == fu && q.v3 == v3) sel.push_back(&q);
        std::stable_sort(sel.begin(), sel.end(), [](const WgQueued* a, const WgQueued* b) {
            return (long long)a->it.cpw * (a->it.H << a->it.lwc) > (long long)b->it.cpw * (b->it.H << b->it.lwc); });
        for (size_t i0 = 0; i0 < sel.size(); i0 += kWgGroupMax) {
            WgGroup g;
            memset(static_cast<void*>(&g), 0, sizeof(g));
            g.n = (int)std::min<size_t>(kWgGroupMax, sel.size() - i0);
            g.tickets = tickets;
            size_t smem = 0;
            int blocks = 0;
            for (int i = 0; i < g.n; ++i) {
                const WgQueued* q = sel[i0 + i];
                g.item[i] = q->it;
                g.first[i] = blocks;
                blocks += q->tiles * q->it.Z;
                smem = std::max(smem, q->smem);
            }
            g.first[g.n] = blocks;
            kernels[cls]<<<blocks, 256, smem, st>>>(g);
            TR_LAUNCH_CHECK();
        }
    }
    return 0;
}

static int wg_group_flush() {
    if (g_wgq.empty()) return 0;
    const int rc = wg_group_launch();
    g_wgq.clear();
    return rc;
}

int rldm_train_wgrad_group(int on) {
    g_wg_group = on;
    return on ? 0 : wg_group_flush();
}

int rldm_train_wgrad_group_flush(void) { return wg_group_flush(); }

int rldm_train_wgrad_group_pending(void) { return (int)g_wgq.size(); }

static int train_wgrad_impl(const rldm_train_conv_desc* d0, const rldm_train_fuse* fu, const float* dy, const float* x, float* dw, float* rows,
                            int rows_ld, int rows_accumulate, float* total, void* stream) {
    RLDM_REQUIRE(d0 && dy && x && dw, "null argument");
    if (flush_reduce()) return 1;                     // (the partial-tile scratch is about to be rewritten)
    rldm_train_conv_desc plain;
    int pad;
    RLDM_REQUIRE(conv_desc_split(d0, &plain, &pad), "bad conv desc");
    const rldm_train_conv_desc* d = &plain;
    TrWgrad p;
    p.dy = dy; p.x = x; p.dw = dw;
    p.B = d->B; p.Win = d->Win; p.Hin = d->Hin; p.Cin = d->Cin; p.N = d->N; p.taps = d->taps; p.stride = d->stride; p.mode = d->mode;
    p.shift = conv_desc_shift(d, pad);
    const int sh = d->mode ? 1 : 0;
    p.Wout = (d->Win << sh) / d->stride; p.Hout = (d->Hin << sh) / d->stride;
    const int P = p.B * p.Wout * p.Hout;
    const int tiles = ((p.N + 63) / 64) * ((p.Cin + 63) / 64) * p.taps;
    // a wave contracts `chunk` pixels into its own partial tile; ~1024 pixels per wave, fewer only to fill the chip
    int chunk = 1024;
    while (chunk > 128 && (long long)tiles * ((P + 4 * chunk - 1) / (4 * chunk)) < 256) chunk >>= 1;
    int splits = (P + 4 * chunk - 1) / (4 * chunk);
    p.chunk = chunk;
    size_t need = (size_t)p.taps * splits * 4 * p.N * p.Cin * sizeof(float);
    // all-taps kernel (see tr_wgrad2_kernel) where the shape allows it: a chunk of WC = 1 << lwc columns
    TrWgrad2 w2{};
    const int lwc = wgrad_v2_shape(d);
    const bool v2 = lwc >= 0;
    if (v2) {
        const int H = p.Hout, W = p.Wout;
        w2.B = p.B; w2.W = W; w2.H = H; w2.Win = p.Win; w2.Hin = p.Hin; w2.Cin = p.Cin; w2.N = p.N; w2.mode = d->mode; w2.lwc = lwc;
        const int WC = 1 << lwc;
        w2.nchunks = p.B * (W / WC);
        const int tiles2 = (p.N / 64) * (p.Cin / 64);
        constexpr int kBlocks = 256;                    // workgroups to aim at
        // (few chunks -- the 32 x 2 level -- : two per workgroup halve the partial tiles for the same kernel time)
        const int cpw_min = w2.nchunks <= 16 ? 2 : 1;
        int Z = std::max(1, std::min(std::max(1, w2.nchunks / cpw_min), (kBlocks + tiles2 - 1) / tiles2));
        w2.cpw = (w2.nchunks + Z - 1) / Z;
        Z = (w2.nchunks + w2.cpw - 1) / w2.cpw;
        w2.pitchA = WC * H + 8;
        w2.pitchB = (p.taps == 9 ? (H + 2) : H) * WC + 8;
        splits = Z;
        need = (size_t)p.taps * Z * p.N * p.Cin * sizeof(float);
    }
    hipStream_t st = (hipStream_t)stream;
    if (deterministic() && v2 && (rows || total)) {
        // deterministic mode: the all-taps kernels add their column sums atomically; the sums come from the fixed-order colsum instead
        // (of the fp32 dy, not of the staged bf16 tile)
        const int rc = rldm_train_colsum(dy, p.B, p.Wout * p.Hout, p.N, rows, rows_ld, rows_accumulate, total, stream);
        if (rc) return rc;
        rows = nullptr;
        total = nullptr;
    }
    if (v2 && g_wg_group) {
        // queued for a grouped launch (tr_wgrad2_group_kernel; K slices: wg_group_launch)
        const bool dw_queued = std::any_of(g_wgq.begin(), g_wgq.end(), [dw](const WgQueued& q) { return q.it.dw == dw; });
        if ((dw_queued || (!g_wgq.empty() && g_wgq_stream != st)) && wg_group_flush()) return 1;
        g_wgq_stream = st;
        const int KP = w2.H << w2.lwc;
        WgQueued q{};
        q.unit = (KP / 128.0) * (p.taps == 9 ? 1.0 : 0.35);
        WgItem& it = q.it;
        it.dy = dy; it.x = x; it.dw = dw; it.rows = rows; it.total = total; it.rows_ld = rows_ld;
        it.B = w2.B; it.W = w2.W; it.H = w2.H; it.Win = w2.Win; it.Hin = w2.Hin; it.Cin = w2.Cin; it.N = w2.N; it.mode = w2.mode;
        it.lwc = w2.lwc; it.cpw = 1; it.nchunks = w2.nchunks; it.Z = 1;         // (cpw / Z: decided per class at the flush)
        const TrFuse f = to_device_fuse(fu, p.Cin, p.N);
        it.x1 = f.x1; it.C0 = f.C0; it.cs0 = f.cs0; it.cs1 = f.cs1; it.gamma = f.gamma; it.beta = f.beta; it.silu = f.silu;
        it.groups = f.groups; it.eps = f.eps;
        q.taps = p.taps; q.fu = fu != nullptr;
        q.v3 = w2.H >= 8 && w2.mode == 0;
        q.tiles = (p.N / 64) * (p.Cin / 64);
        q.part_floats = 0;
        // (Z == 1: the tile goes through LDS into dw)
        q.smem = wgrad2_lds_bytes(p.taps, w2.H, w2.lwc, w2.pitchA, w2.pitchB, fu != nullptr, p.B, q.v3, true);
        if (rows && !rows_accumulate && launch_zero2d(rows, rows_ld, p.N, p.B, st)) return 1;
        g_wgq.push_back(q);
        return 0;
    }
    float* scratch = nullptr;
    if (tr_scratch(kWgradPartials, need, 0, false, st, reinterpret_cast<void**>(&scratch))) return 1;
    p.dw = scratch;
    if (v2) {
        w2.dy = dy; w2.x = x; w2.part = scratch;
        w2.dw = p.taps == 9 || deterministic() ? nullptr : dw;  // (measured: 3x3 tiles are 9x larger, their 38 MB of atomics lose to the
                                                                //  partial tiles + reduction launch by 10-30 %; 1x1 wins 25-35 %;
                                                                //  deterministic mode: always partial tiles, summed in slice order)
        w2.rows = rows; w2.rows_ld = rows_ld; w2.total = total;
        if (rows && !rows_accumulate && launch_zero2d(rows, rows_ld, p.N, p.B, st)) return 1;
        const size_t smem = wgrad2_lds_bytes(p.taps, w2.H, w2.lwc, w2.pitchA, w2.pitchB, fu != nullptr, p.B, false, w2.dw != nullptr);
        typedef void (*DirectKernel)(const TrWgrad2, const TrFuse);
        static const DirectKernel kernels[4] = {tr_wgrad2_kernel<9>, tr_wgrad2_kernel<1>, tr_wgrad2_kernel<9, true>, tr_wgrad2_kernel<1, true>};
        static bool attr = false;
        if (wgrad2_allow_lds(kernels, 160 * 1024, &attr)) return 1;
        const dim3 grid((p.N / 64) * (p.Cin / 64), splits);
        kernels[(fu ? 2 : 0) | (p.taps == 9 ? 0 : 1)]<<<grid, 256, smem, st>>>(w2, to_device_fuse(fu, p.Cin, p.N));
        TR_LAUNCH_CHECK();
        if (!w2.dw) {
            if (g_defer_reduce) {                     // rides on the next conv launch (or is flushed by whatever comes first)
                g_red.part = scratch; g_red.dw = dw; g_red.slices = splits; g_red.N = p.N; g_red.Cin = p.Cin; g_red.taps = p.taps; g_red.st = st;
            } else
                tr_wgrad_reduce_vec_kernel<<<nblk((size_t)p.N * p.Cin * p.taps / 4), 256, 0, st>>>(scratch, splits, p.N, p.Cin, p.taps, dw);
        }
        TR_LAUNCH_CHECK();
        return 0;
    }
    RLDM_REQUIRE(!fu, "rldm_train_wgrad_fused: not an all-taps shape");
    if (rows || total) {                              // the one-tap kernel does not carry the column sums
        const int rc = rldm_train_colsum(dy, p.B, p.Wout * p.Hout, p.N, rows, rows_ld, rows_accumulate, total, stream);
        if (rc) return rc;
    }
    tr_wgrad_kernel<<<dim3(((p.N + 63) / 64) * ((p.Cin + 63) / 64), p.taps, splits), 256, 0, st>>>(p);
    TR_LAUNCH_CHECK();
    tr_wgrad_reduce_kernel<<<nblk((size_t)p.N * p.Cin * p.taps), 256, 0, st>>>(scratch, splits * 4, p.N, p.Cin, p.taps, dw);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_wgrad_bias(const rldm_train_conv_desc* d, const float* dy, const float* x, float* dw, float* rows, int rows_ld,
                          int rows_accumulate, float* total, void* stream) {
    return train_wgrad_impl(d, nullptr, dy, x, dw, rows, rows_ld, rows_accumulate, total, stream);
}

int rldm_train_wgrad_fused(const rldm_train_conv_desc* d, const rldm_train_fuse* fu, const float* dy, const float* x, float* dw, float* rows,
                           int rows_ld, int rows_accumulate, float* total, void* stream) {
    RLDM_REQUIRE(d && fu && rldm_train_wgrad_fused_ok(d, fu), "rldm_train_wgrad_fused: shape not supported (ask rldm_train_wgrad_fused_ok)");
    return train_wgrad_impl(d, fu, dy, x, dw, rows, rows_ld, rows_accumulate, total, stream);
}

int rldm_train_wgrad(const rldm_train_conv_desc* d, const float* dy, const float* x, float* dw, void* stream) {
    return rldm_train_wgrad_bias(d, dy, x, dw, nullptr, 0, 0, nullptr, stream);
}

int rldm_train_linear_rows_wgrad(const float* dy, int ldy, const float* x, int ldx, int B, int N, int K, float* dw, float* dbias,
                                 void* stream) {
    RLDM_REQUIRE(dy && x && dw, "null argument");
    RLDM_REQUIRE(B >= 1 && K % 4 == 0 && ldx % 4 == 0, "K a multiple of 4");
    tr_linear_rows_wgrad_kernel<<<nblk((size_t)N * (K / 4)), 256, 0, (hipStream_t)stream>>>(dy, ldy, x, ldx, B, N, K, dw, dbias);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_colsum(const float* dy, int B, int npix, int N, float* rows, int rows_ld, int rows_accumulate, float* total,
                      void* stream) {
    RLDM_REQUIRE(dy && (rows || total), "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (deterministic()) {
        const int S = (npix + 255) / 256;
        float* part = nullptr;
        if (det_partials((size_t)B * S * N * sizeof(float), st, reinterpret_cast<void**>(&part))) return 1;
        tr_colsum_kernel<true><<<dim3((N + 63) / 64, B, S), 256, 0, st>>>(dy, npix, N, part, 0, nullptr);
        tr_colsum_finish_kernel<<<nblk((size_t)N), 256, 0, st>>>(part, B, S, N, rows, rows_ld, rows_accumulate, total);
        TR_LAUNCH_CHECK();
        return 0;
    }
    if (rows && !rows_accumulate && launch_zero2d(rows, rows_ld, N, B, st)) return 1;
    tr_colsum_kernel<false><<<dim3((N + 63) / 64, B, (npix + 255) / 256), 256, 0, st>>>(dy, npix, N, rows, rows_ld, total);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
