// train_conv.hip -- the convolutions of the training step, forward and data gradient (rldm_train_conv, rldm_train_conv_fused), and the
// Linear layers on a handful of rows (rldm_train_linear_rows).  Operand formats: train.hip's header.
//   tr_conv_kernel        conv 3x3 / 1x1 (circular W, zero H; stride 1 | 2; nearest-x2 or zero-insertion of the input) + bias + per-sample
//                         row (time embedding) + residual, operands straight from global memory: any shape, and every Linear (W = H = 1).
//   tr_conv_lds_kernel    the same through LDS stages for Cin % 32 == 0, split over K when the launch cannot fill the chip.
//   tr_conv_halo_kernel   stride-1 3x3 convs that fill the chip: a chunk's pixel tile staged once with its halo for all nine taps.
//   fused forms (TrFuse)  GroupNorm (+ SiLU) of a one- or two-source input while staging; tr_tile_epilogue: the output's statistics, or the
//                         GroupNorm-backward transform and its sums; extra z-planes carry train_wgrad.hip's pending reduction.
//   DET forms             rldm_train_deterministic: never split over K; the epilogue's sums leave as a partial row per tile, folded behind it.
// train_conv_impl picks the instance from one table: (halo | CK 64 | CK 32) x (wide | narrow) x (plain | fused | deterministic).
#include "train_common.h"

#include <algorithm>

using namespace rldm::train;

namespace {

// ---- convolution / linear (forward and data gradient) ---------------------------------------------------------------
struct TrConv {
    const float* x; const bf16_t* w; const float* bias; const float* rowadd; const float* res; float* y;
    int B, Win, Hin, Cin, Cin_pad, Wout, Hout, N, taps, stride, mode, rowadd_ld, accumulate, shift;
};

// Epilogue of a fused conv over the finished fp32 tile in LDS (tile[pl * (BN + 1) + cl], 64 pixels of ONE image x BN channels), run by
// the workgroup's 256 threads:
// thread (channel cl = tid % BN, pixel group tid / BN) walks its pixels: + bias / row / residual (add_terms), the GroupNorm-backward
// transform where asked, the store (coalesced along the channels), and the per-channel sums, which reach cs_out / gs_out as one atomic
// per (workgroup, channel, component).  colacc: [2 * BN] floats of LDS.
template <int BN, bool DET = false>
__device__ inline void tr_tile_epilogue(const float* tile, float* colacc, const float4* ce, const TrConv& p, const TrFuse& f, int px0,
                                        int n0, int img, bool add_terms, bool store_y) {
    // thread (channel quad cq = tid % (BN / 4), pixel group tid / (BN / 4)): 16-byte global accesses, all of a thread's loads in flight
    // at once (the 4-byte form of this pass -- a channel per thread, 32 pixels in two batches -- was ~5 us of every fused launch)
    constexpr int PT = 64, NT = 256;
    constexpr int NQ = BN / 4, NPG = NT / NQ, IT = PT / NPG;        // BN = 128: 32 quads x 8 groups, 8 pixels per thread
    const int tid = threadIdx.x, cq = tid % NQ, pg = tid / NQ, cl = 4 * cq, ch = n0 + cl, N = p.N;
    for (int e = tid; e < 2 * BN; e += NT) colacc[e] = 0.f;
    __syncthreads();
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    // (DET) the canonical partial of rldm_train_deterministic: lane k of 16 adds the tile's pixels k, k + 16, k + 32, k + 48 in that order;
    // a thread walks pixels pg + u NPG, so it holds lanes pg + j NPG (NL = 1 or 2 of them)
    constexpr int NL = DET ? 16 / NPG : 1;
    f32x4 d1[NL], d2[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) { d1[j] = f32x4{0.f, 0.f, 0.f, 0.f}; d2[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (ch < N) {                                                   // (N % 4 == 0: a quad is inside or outside)
        f32x4 addc = {0.f, 0.f, 0.f, 0.f};
        if (add_terms) {
            if (p.bias) addc += tr_load4(p.bias + ch);
            if (p.rowadd) addc += *reinterpret_cast<const f32x4*>(p.rowadd + (size_t)img * p.rowadd_ld + ch);
        }
        const bool gn = f.gs_out != nullptr, act = gn && f.gsilu != 0;
        float4 c4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c4[q] = gn ? ce[cl + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* __restrict__ gsrc = nullptr;
        int gld = 0;
        if (gn) {                                                   // (G0 % 4 == 0: the quad lies in one source)
            if (ch < f.G0) { gsrc = f.g0 + ch; gld = f.G0; }
            else { gsrc = f.g1 + (ch - f.G0); gld = N - f.G0; }
        }
        const float* __restrict__ rsrc = (add_terms && p.res) ? p.res + ch : nullptr;
        float* __restrict__ ydst = p.y + ch;
        f32x4 rv[IT], gv[IT];
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const size_t gp = (size_t)px0 + pg + u * NPG;
            rv[u] = rsrc ? *reinterpret_cast<const f32x4*>(rsrc + gp * N) : f32x4{0.f, 0.f, 0.f, 0.f};
            gv[u] = gn ? *reinterpret_cast<const f32x4*>(gsrc + gp * gld) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int pl = pg + u * NPG;
            const size_t gp = (size_t)px0 + pl;
            const float* tr_ = tile + pl * (BN + 1) + cl;
            f32x4 v = {tr_[0], tr_[1], tr_[2], tr_[3]};
            v += addc + rv[u];
            if (gn) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float g = gv[u][q], xh = (g - c4[q].z) * c4[q].w;
                    if (act) {
                        const float z = g * c4[q].x + c4[q].y, sg = tr_sigmoid(z);
                        v[q] *= sg * (1.f + z * (1.f - sg));
                    }
                    if constexpr (DET) {
                        d1[u % NL][q] = det_add(d1[u % NL][q], v[q]);
                        d2[u % NL][q] = det_add(d2[u % NL][q], det_mul(v[q], xh));
                    } else {
                        s1[q] += v[q];
                        s2[q] += v[q] * xh;
                    }
                }
                *reinterpret_cast<f32x4*>(ydst + gp * N) = v;
            } else {
                if constexpr (DET) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        d1[u % NL][q] = det_add(d1[u % NL][q], v[q]);
                        d2[u % NL][q] = det_add(d2[u % NL][q], det_mul(v[q], v[q]));
                    }
                } else {
                    s1 += v;
                    s2 += v * v;
                }
                if (store_y) *reinterpret_cast<f32x4*>(ydst + gp * N) = v;
            }
        }
    }
    if constexpr (DET) {
        // the 16 lanes through LDS (over the tile, which every thread has read by now), folded k = 0 .. 15 by one thread per (channel,
        // component); the tile's row of partials goes to scratch and tr_fold_rows_kernel adds the tiles of an image in tile order
        float* lanes = const_cast<float*>(tile);                    // [16][2 * BN]  (16 * 2 BN <= 64 (BN + 1) floats)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NL; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                lanes[(pg + j * NPG) * (2 * BN) + 2 * (cl + q)] = d1[j][q];
                lanes[(pg + j * NPG) * (2 * BN) + 2 * (cl + q) + 1] = d2[j][q];
            }
        __syncthreads();
        for (int e = tid; e < 2 * BN; e += NT) {
            const int c2 = n0 + (e >> 1);
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) a = det_add(a, lanes[k * (2 * BN) + e]);
            if (c2 < N) f.part[((size_t)(px0 >> 6) * N + c2) * 2 + (e & 1)] = a;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        atomicAdd(&colacc[2 * (cl + q)], s1[q]);
        atomicAdd(&colacc[2 * (cl + q) + 1], s2[q]);
    }
    __syncthreads();
    float* out = f.gs_out ? f.gs_out : f.cs_out;
    for (int e = tid; e < 2 * BN; e += NT) {
        const int c2 = n0 + (e >> 1);
        if (c2 < N) unsafeAtomicAdd(out + ((size_t)img * N + c2) * 2 + (e & 1), colacc[e]);
    }
}

// D[channel][pixel]: lane (pixel l & 31, half l >> 5) holds channels (r & 3) + 8 (r >> 2) + 4 half of its pixel.
// A wave owns 32 pixels x 64 channels (one pixel fragment feeds two MFMAs); a workgroup 64 pixels x 128 channels.
template <bool FAST>
__global__ __launch_bounds__(256) void tr_conv_kernel(const TrConv p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, kg = lane >> 5;
    const int P = p.B * p.Wout * p.Hout;
    const int px = blockIdx.x * 64 + (wave & 1) * 32 + l31;
    const int n0 = blockIdx.y * 128 + (wave >> 1) * 64;
    if (n0 >= p.N) return;
    const bool pxok = px < P;
    const int pc = pxok ? px : 0;
    const int ho = pc % p.Hout, t1 = pc / p.Hout, wo = t1 % p.Wout, b = t1 / p.Wout;
    const int r0 = n0 + l31, r1 = r0 + 32;                            // this lane's weight rows (A operands)
    const bool ok0 = r0 < p.N, ok1 = r1 < p.N;
    const size_t rstride = (size_t)p.taps * p.Cin_pad;
    const bf16_t* w0 = p.w + (size_t)(ok0 ? r0 : 0) * rstride + 8 * kg;
    const bf16_t* w1 = p.w + (size_t)(ok1 ? r1 : 0) * rstride + 8 * kg;
    const bool vec = (p.Cin & 3) == 0;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    for (int t = 0; t < p.taps; ++t) {
        const int dw = p.taps == 9 ? t / 3 - 1 : 0, dh = p.taps == 9 ? t % 3 - 1 : 0;
        const int sp = pxok ? src_pixel(b, wo, ho, dw, dh, p.stride, p.mode, p.Win, p.Hin, p.shift) : -1;
        const float* xrow = p.x + (size_t)(sp < 0 ? 0 : sp) * p.Cin + 8 * kg;
        const size_t toff = (size_t)t * p.Cin_pad;
        if (FAST) {
            // Cin % 16 == 0: branch-free body, four k-steps of loads in flight (rows past N are computed on row 0's
            // weights and never stored; a zero-padded tap multiplies by 0)
            const float live = sp < 0 ? 0.f : 1.f;
            const bf16_t* wa = w0 + toff;
            const bf16_t* wb = w1 + toff;
#pragma unroll 4
            for (int c0 = 0; c0 < p.Cin_pad; c0 += 16) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(wa + c0), a1 = *reinterpret_cast<const uint4*>(wb + c0);
                const float4 x0 = *reinterpret_cast<const float4*>(xrow + c0), x1 = *reinterpret_cast<const float4*>(xrow + c0 + 4);
                uint4 u;
                u.x = rldm::pack_bf16x2(x0.x * live, x0.y * live); u.y = rldm::pack_bf16x2(x0.z * live, x0.w * live);
                u.z = rldm::pack_bf16x2(x1.x * live, x1.y * live); u.w = rldm::pack_bf16x2(x1.z * live, x1.w * live);
                const bf16x8 bv = __builtin_bit_cast(bf16x8, u);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), bv, acc1, 0, 0, 0);
            }
        } else {
            for (int c0 = 0; c0 < p.Cin_pad; c0 += 16) {
                uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0;
                if (ok0) a0 = *reinterpret_cast<const uint4*>(w0 + toff + c0);
                if (ok1) a1 = *reinterpret_cast<const uint4*>(w1 + toff + c0);
                const int valid = sp < 0 ? 0 : p.Cin - (c0 + 8 * kg);
                const bf16x8 bv = load_bf16x8_from_f32(xrow + c0, valid, vec);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), bv, acc1, 0, 0, 0);
            }
        }
    }
    if (!pxok) return;
    float* yrow = p.y + (size_t)px * p.N;
    const float* rrow = p.res ? p.res + (size_t)px * p.N : nullptr;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = n0 + 32 * h + (r & 3) + 8 * (r >> 2) + 4 * kg;
            if (ch >= p.N) continue;
            float v = h ? acc1[r] : acc0[r];
            if (p.bias) v += p.bias[ch];
            if (p.rowadd) v += p.rowadd[(size_t)b * p.rowadd_ld + ch];
            if (rrow) v += rrow[ch];
            if (p.accumulate) v += yrow[ch];
            yrow[ch] = v;
        }
}

// LDS-staged variant for Cin % CK == 0 (CK = 32 | 64 channels per stage): the workgroup (64 pixels x 128 channels) stages the
// pixel tile [64][CK] (fp32 -> bf16 on the way) and the weight tile [128][CK] with coalesced pieces per thread.  A stage
// costs one memory latency (~1.5 us measured: activations of a level live in the Infinity Cache, not in L2) against 0.1 us
// of MFMAs, so the global loads of the next stage are kept in flight in registers during this stage's MFMAs.  (Three stages in flight
// were measured on the low-resolution launches and changed nothing -- a 4-stage 1x1 conv 9.6 against 9.4 us, the 64x4 level's 3x3 convs
// 19.0 against 21.6 us, the step 798 against 796 samples/s: those launches are bound by launch + first-touch + drain latency.)
// Row pitch CK * 2 + 16 bytes: an odd number of 16-byte slots, conflict-free ds_read_b128.
// (round 5) FU: the fused form (TrFuse) -- GroupNorm (+ SiLU) of a one- or two-source input while staging, and the tile epilogue
// (tr_tile_epilogue: output statistics or the GroupNorm-backward transform + sums), in split-K launches run by each tile's last arriver.
template <int CK, int BN, bool FU = false, bool DET = false>
__global__ __launch_bounds__(256) void tr_conv_lds_kernel(const TrConv p, const TrFuse f) {
    static_assert(BN == 64 || BN == 128, "channel tile");
    constexpr int TPR = 256 / BN, NR = BN / 64;     // threads per weight row of a stage; 32-channel MFMA rows per wave
    constexpr int PITCH = CK + 8;                   // bf16 elements
    constexpr int XV = CK / 32;                     // float4 pairs per thread for x (4 threads per pixel row, CK / 4 channels each)
    constexpr int WV = CK / (8 * TPR);              // uint4 per thread for w
    // one buffer: the two stage tiles during the K loop, the fp32 output tile [64][BN + 1] of the split-K epilogue afterwards
    constexpr int STAGE_BYTES = (64 + BN) * PITCH * 2, TILE_BYTES = 64 * (BN + 1) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char raw[STAGE_BYTES > TILE_BYTES ? STAGE_BYTES : TILE_BYTES];
    bf16_t* const sX = reinterpret_cast<bf16_t*>(raw);
    bf16_t* const sW = sX + 64 * PITCH;
    __shared__ float2 sSc[FU ? 768 : 1];                            // (FU) input GroupNorm: (a, b) per input channel
    __shared__ float4 sCe[FU ? BN : 1];                             // (FU) epilogue GroupNorm: (a, b, mean, rstd) per tile channel
    __shared__ float sCol[FU ? 2 * BN : 1];
    __shared__ int sLast;
    // (native vector types: arrays of HIP's uint4 / float4 structs are not split into registers and went through scratch;
    //  no lambda may capture the by-value argument `p` by reference either: that copies the struct to scratch)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int ksplit = f.rblocks ? f.rz0 : (int)gridDim.z;          // (z-planes from rz0 on carry the rider)
    if ((int)blockIdx.z >= ksplit) {
        const int rb = ((int)blockIdx.z - ksplit) * (int)(gridDim.x * gridDim.y) + (int)(blockIdx.y * gridDim.x + blockIdx.x);
        if (rb < f.rblocks) tr_wgrad_reduce_items(f.rpart, f.rslices, f.rN, f.rCin, f.rtaps, f.rdw, rb, f.rblocks, 256);
        return;
    }
    const int Cin = p.Cin, Cin_pad = p.Cin_pad, taps = p.taps, Wout = p.Wout, Hout = p.Hout, N = p.N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kg = lane >> 5;
    const int P = p.B * Wout * Hout;
    const int px0 = blockIdx.x * 64, n0 = blockIdx.y * BN;
    const int img = FU ? px0 / (Wout * Hout) : 0;                   // (FU: a tile lies inside one image)
    const bool in_gn = FU && f.cs0 != nullptr;
    const int fC0 = FU ? f.C0 : Cin;
    // staging roles
    const int spx = tid >> 2, spart = tid & 3;      // x: pixel row of the tile, quarter of the CK channels
    const int swr = tid / TPR, shalf = tid % TPR;   // w: weight row of the tile, 1 / TPR of the CK channels
    const int gpx = px0 + spx;
    const bool gpx_ok = gpx < P;
    const int pc = gpx_ok ? gpx : 0;
    const int sho = pc % Hout, st1 = pc / Hout, swo = st1 % Wout, sb = st1 / Wout;
    const int wrow = n0 + swr;
    const bf16_t* wptr = p.w + (size_t)(wrow < N ? wrow : 0) * taps * Cin_pad + shalf * (CK / TPR);     // walks [tap][chunk]
    const float* const xbase = p.x + spart * (CK / 4);
    const int nck = Cin / CK, niter = taps * nck;
    const int wskip = Cin_pad - Cin;                // weight rows are padded to 16 channels per tap
    // stage walker: (tap, chunk) advance without divisions; the tap's source pixel is looked up when the tap changes
    int tap = 0, cc = 0;
    const float* xs = xbase;
    float live = 0.f;
    int sp_cur = 0, scc = 0;                        // (FU) source pixel of the current tap; chunk of the data in the staging registers
    const float* const x1p = FU ? f.x1 : nullptr;
    auto new_tap = [&]() __attribute__((always_inline)) {
        const int dw = taps == 9 ? tap / 3 - 1 : 0, dh = taps == 9 ? tap % 3 - 1 : 0;
        const int sp = gpx_ok ? src_pixel(sb, swo, sho, dw, dh, p.stride, p.mode, p.Win, p.Hin, p.shift) : -1;
        live = sp < 0 ? 0.f : 1.f;
        sp_cur = sp < 0 ? 0 : sp;
        xs = xbase + (size_t)sp_cur * Cin;
    };
    // split K: workgroup z of gridDim.z contracts stages [it0, it1) and adds its partial tile to y atomically (y zeroed by the
    // launcher; z == 0 carries bias / row / residual).  The low-resolution levels have 32 - 128 output tiles for 36 - 72
    // serial stages of ~0.7 us each: latency, not work, was their whole cost.
    const int it0 = (int)((long long)niter * blockIdx.z / ksplit), it1 = (int)((long long)niter * (blockIdx.z + 1) / ksplit);
    tap = it0 / nck;
    cc = it0 - tap * nck;
    wptr += (size_t)tap * Cin_pad + cc * CK;
    new_tap();
    xs += cc * CK;
    f32x4 xr[XV][2];                                // the one stage in flight: its data, its tap's liveness, (FU) its chunk
    u32x4 wr[WV];
    float lvs;
    int sccs;
    auto fetch = [&]() __attribute__((always_inline)) {
        lvs = live;
        const float* src = xs;
        if constexpr (FU) {                         // two sources: the chunk lies in one of them (C0 % CK == 0)
            const int c = cc * CK + spart * (CK / 4);
            src = c < fC0 ? p.x + (size_t)sp_cur * fC0 + c : x1p + (size_t)sp_cur * (Cin - fC0) + (c - fC0);
            sccs = cc;
        }
#pragma unroll
        for (int q = 0; q < XV; ++q) {
            xr[q][0] = reinterpret_cast<const f32x4*>(src)[2 * q];
            xr[q][1] = reinterpret_cast<const f32x4*>(src)[2 * q + 1];
        }
#pragma unroll
        for (int q = 0; q < WV; ++q) wr[q] = reinterpret_cast<const u32x4*>(wptr)[q];
        xs += CK;
        wptr += CK;
        if (++cc == nck) {
            cc = 0;
            ++tap;
            wptr += wskip;
            new_tap();
        }
    };
    auto stash = [&]() __attribute__((always_inline)) {
        const float lv = lvs;
#pragma unroll
        for (int q = 0; q < XV; ++q) {
            f32x4 a = xr[q][0], b = xr[q][1];
            if constexpr (FU) {
                if (in_gn) {                        // GroupNorm (+ SiLU) of the staged values (zero padding applies to the result: lv below)
                    const float2* co = sSc + sccs * CK + spart * (CK / 4) + 8 * q;
                    const bool act = f.silu != 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float2 c0_ = co[e], c1_ = co[4 + e];
                        float z0 = a[e] * c0_.x + c0_.y, z1 = b[e] * c1_.x + c1_.y;
                        if (act) { z0 *= tr_sigmoid(z0); z1 *= tr_sigmoid(z1); }
                        a[e] = z0; b[e] = z1;
                    }
                }
            }
            u32x4 u;
            u.x = rldm::pack_bf16x2(a.x * lv, a.y * lv); u.y = rldm::pack_bf16x2(a.z * lv, a.w * lv);
            u.z = rldm::pack_bf16x2(b.x * lv, b.y * lv); u.w = rldm::pack_bf16x2(b.z * lv, b.w * lv);
            *reinterpret_cast<u32x4*>(sX + spx * PITCH + spart * (CK / 4) + 8 * q) = u;
        }
#pragma unroll
        for (int q = 0; q < WV; ++q) *reinterpret_cast<u32x4*>(sW + swr * PITCH + shalf * (CK / TPR) + 8 * q) = wr[q];
    };
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const bf16_t* bx = sX + ((wave & 1) * 32 + l31) * PITCH + 8 * kg;
    const bf16_t* aw0 = sW + ((wave >> 1) * (BN / 2) + l31) * PITCH + 8 * kg;
    const bf16_t* aw1 = aw0 + (NR == 2 ? 32 : 0) * PITCH;
    if (it0 < it1) fetch();
    if constexpr (FU) {
        // (behind the first stage's loads; a K split only needs the chunks of its own stages; visible after the loop's first barrier)
        if (in_gn) {
            const bool all = it1 - it0 >= nck;
            const int c_lo = all ? 0 : (it0 % nck) * CK, c_hi = all ? Cin : c_lo + (it1 - it0) * CK;
            tr_gn_coeffs(sSc, c_lo, min(c_hi, Cin), f.cs0, f.cs1, fC0, Cin, img, f.groups, f.eps, p.Win * p.Hin, f.gamma, f.beta);
            if (c_hi > Cin) tr_gn_coeffs(sSc, 0, c_hi - Cin, f.cs0, f.cs1, fC0, Cin, img, f.groups, f.eps, p.Win * p.Hin, f.gamma, f.beta);
        }
        if (f.gs_out && ksplit == 1)
            tr_gn_coeffs_tile(sCe, BN, n0, f.gcs0, f.gcs1, f.G0, N, img, f.ggroups, f.geps, Wout * Hout, f.ggamma, f.gbeta);
    }
    for (int it = it0; it < it1; ++it) {
        __syncthreads();                            // everyone is done reading the previous stage
        stash();
        __syncthreads();
        if (it + 1 < it1) fetch();                  // the registers just copied out are requested again: in flight during the MFMAs
#pragma unroll
        for (int ks = 0; ks < CK / 16; ++ks) {
            const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bx + 16 * ks);
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(aw0 + 16 * ks);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bv, acc0, 0, 0, 0);
            if (NR == 2) {
                const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(aw1 + 16 * ks);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bv, acc1, 0, 0, 0);
            }
        }
    }
    if (!DET && ksplit > 1) {                       // (the deterministic instances are never launched split: no atomics in them)
        // through LDS so that the atomics run along the channels (one cache line per 32 lanes; lane = pixel would touch 64 lines
        // per instruction: measured 4x slower than not splitting at all)
        float* tile = reinterpret_cast<float*>(raw);
        __syncthreads();
        {
            float* trow = tile + ((wave & 1) * 32 + l31) * (BN + 1) + (wave >> 1) * (BN / 2);
#pragma unroll
            for (int h = 0; h < NR; ++h)
#pragma unroll
                for (int r = 0; r < 16; ++r) trow[32 * h + 8 * (r >> 2) + 4 * kg + (r & 3)] = h ? acc1[r] : acc0[r];
        }
        __syncthreads();
        const bool first = blockIdx.z == 0;
        const int HW = p.Wout * p.Hout;
        for (int e = tid; e < 64 * BN; e += 256) {
            const int pl = e / BN, cl = e % BN;
            const int gp = px0 + pl, ch = n0 + cl;
            if (gp >= P || ch >= p.N) continue;
            float u = tile[pl * (BN + 1) + cl];
            if (first) {
                if (p.bias) u += p.bias[ch];
                if (p.rowadd) u += p.rowadd[(size_t)(gp / HW) * p.rowadd_ld + ch];
                if (p.res) u += p.res[(size_t)gp * p.N + ch];
            }
            unsafeAtomicAdd(p.y + (size_t)gp * p.N + ch, u);
        }
        if constexpr (FU) {
            if (f.cs_out || f.gs_out) {
                // the tile's last arriver runs the epilogue over the finished sums.  The partial tiles travel as device-scope atomics --
                // performed at the coherence point, never dirty in an L2 -- so "published" = every wave has its atomics acknowledged
                // (s_waitcnt vmcnt(0)) before one lane draws the ticket: no write-back fence (cdna_hip_programming.md prices it at 1.7 -
                // 6.5 us per workgroup).  The last arriver added to every line of the tile itself (an atomic drops the line from its L2)
                // and never read one (nothing in its L1): it re-reads the tile with L1-bypassing loads, no invalidate.
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    unsigned* tk = f.tickets + blockIdx.y * gridDim.x + blockIdx.x;
                    const unsigned t = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    const int last = (int)t == ksplit - 1;
                    if (last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sLast = last;
                }
                __syncthreads();
                if (!sLast) return;
                // (round 6) the argument above rests on what an atomic does to a line of the issuing XCD's L2, which nothing documents:
                // the ONE workgroup per tile that re-reads the sums pairs the release on the ticket with an agent-scope acquire (an
                // invalidate of what its caches may hold of the tile) before it does.
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                if (f.gs_out) tr_gn_coeffs_tile(sCe, BN, n0, f.gcs0, f.gcs1, f.G0, N, img, f.ggroups, f.geps, Wout * Hout, f.ggamma, f.gbeta);
                if ((N & 3) == 0) {
                    for (int e = tid; e < 64 * (BN / 4); e += 256) {
                        const int pl = e / (BN / 4), cl = (e % (BN / 4)) * 4;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (n0 + cl < N) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.y + (size_t)(px0 + pl) * N + n0 + cl));
#pragma unroll
                        for (int q = 0; q < 4; ++q) tile[pl * (BN + 1) + cl + q] = v[q];
                    }
                } else {
                    for (int e = tid; e < 64 * BN; e += 256) {
                        const int pl = e / BN, cl = e % BN;
                        const int ch = n0 + cl;
                        tile[pl * (BN + 1) + cl] = ch < N ? __hip_atomic_load(p.y + (size_t)(px0 + pl) * N + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                    }
                }
                __syncthreads();
                tr_tile_epilogue<BN>(tile, sCol, sCe, p, f, px0, n0, img, false, false);
            }
        }
        return;
    }
    if constexpr (FU) {
        if (f.cs_out || f.gs_out) {
            float* tile = reinterpret_cast<float*>(raw);
            __syncthreads();
            float* trow = tile + ((wave & 1) * 32 + l31) * (BN + 1) + (wave >> 1) * (BN / 2);
#pragma unroll
            for (int h = 0; h < NR; ++h)
#pragma unroll
                for (int r = 0; r < 16; ++r) trow[32 * h + 8 * (r >> 2) + 4 * kg + (r & 3)] = h ? acc1[r] : acc0[r];
            __syncthreads();
            tr_tile_epilogue<BN, DET>(tile, sCol, sCe, p, f, px0, n0, img, true, true);
            return;
        }
    }
    const int px = px0 + (wave & 1) * 32 + l31;
    if (px >= P) return;
    const int b = px / (p.Wout * p.Hout);
    const int nb = n0 + (wave >> 1) * (BN / 2);
    float* yrow = p.y + (size_t)px * p.N;
    const float* rrow = p.res ? p.res + (size_t)px * p.N : nullptr;
#pragma unroll
    for (int h = 0; h < NR; ++h)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
            const int ch = nb + 32 * h + 8 * (r >> 2) + 4 * kg;       // 4 consecutive channels per register quad
            if (ch >= p.N) continue;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = h ? acc1[r + e] : acc0[r + e];
            if (ch + 3 < p.N && (p.N & 3) == 0) {
                if (p.bias) { const f32x4 t = tr_load4(p.bias + ch); v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3]; }
                if (p.rowadd) { const float4 t = *reinterpret_cast<const float4*>(p.rowadd + (size_t)b * p.rowadd_ld + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
                if (rrow) { const float4 t = *reinterpret_cast<const float4*>(rrow + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
                if (p.accumulate) { const float4 t = *reinterpret_cast<const float4*>(yrow + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
                *reinterpret_cast<float4*>(yrow + ch) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (ch + e >= p.N) continue;
                    float u = v[e];
                    if (p.bias) u += p.bias[ch + e];
                    if (p.rowadd) u += p.rowadd[(size_t)b * p.rowadd_ld + ch + e];
                    if (rrow) u += rrow[ch + e];
                    if (p.accumulate) u += yrow[ch + e];
                    yrow[ch + e] = u;
                }
            }
        }
}

// Halo variant for the stride-1, mode-0 3x3 convs whose launch fills the chip (levels 0 / 1: forward and data gradient): the
// kernel above re-stages its 64-pixel tile for every tap (9 x 16 KB of fp32 per 64-channel chunk and workgroup -- at level 0
// 302 MB through L2 in 26 us, which is what bounds it).  Here a 64-channel chunk's tile is staged ONCE with its halo --
// (64 / H + 2) azimuth columns x (H + 2) beams, circular in azimuth, zero rows above and below -- and the nine taps read
// their B fragments from it at a uniform row offset dw * (H + 2) + dh; only the weight tile is staged per tap.  x traffic
// and fp32->bf16 conversions drop 5x.  Stage order: chunk-major, tap fastest.
template <int BN, bool FU = false, bool DET = false>
__global__ __launch_bounds__(256) void tr_conv_halo_kernel(const TrConv p, const TrFuse f) {
    static_assert(BN == 64 || BN == 128, "channel tile");
    constexpr int CK = 64;
    constexpr int PT = 64;                          // pixel tile
    constexpr int NT = 256;                         // threads: PT / 32 pixel groups x 2 channel halves of waves
    constexpr int TPR = NT / BN, NR = BN / 64;
    constexpr int PITCH = CK + 8;
    constexpr int WV = CK / (8 * TPR);
    constexpr int MAXHP = 136;                      // (PT / H + 2) * (H + 2) for H = 2 .. 32
    // (FU: one buffer, the fp32 output tile [PT][BN + 1] of the fused epilogue afterwards)
    constexpr int STAGE_BYTES = (MAXHP + BN) * PITCH * 2, TILE_BYTES = FU ? PT * (BN + 1) * 4 : 0;
    __shared__ __attribute__((aligned(16))) unsigned char hraw[STAGE_BYTES > TILE_BYTES ? STAGE_BYTES : TILE_BYTES];
    bf16_t* const sXh = reinterpret_cast<bf16_t*>(hraw);
    bf16_t* const sW = sXh + MAXHP * PITCH;
    __shared__ float2 sSc[FU ? 768 : 1];
    __shared__ float4 sCe[FU ? BN : 1];
    __shared__ float sCol[FU ? 2 * BN : 1];
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    if (f.rblocks && (int)blockIdx.z >= f.rz0) {                    // the rider's z-planes
        const int rb = ((int)blockIdx.z - f.rz0) * (int)(gridDim.x * gridDim.y) + (int)(blockIdx.y * gridDim.x + blockIdx.x);
        if (rb < f.rblocks) tr_wgrad_reduce_items(f.rpart, f.rslices, f.rN, f.rCin, f.rtaps, f.rdw, rb, f.rblocks, NT);
        return;
    }
    const int Cin = p.Cin, Cin_pad = p.Cin_pad, W = p.Wout, H = p.Hout, N = p.N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kg = lane >> 5;
    const int px0 = blockIdx.x * PT, n0 = blockIdx.y * BN;
    const int WCt = PT / H, HP2 = H + 2, HP = (WCt + 2) * HP2;
    const int b = px0 / (W * H), w0 = (px0 / H) % W;                 // the tile = WCt whole columns of image b
    const bool in_gn = FU && f.cs0 != nullptr;
    const int fC0 = FU ? f.C0 : Cin;
    const float* const x1p = FU ? f.x1 : nullptr;
    // halo staging roles: pass j: halo pixel hp = PT j + (tid >> 2), quarter (tid & 3) of the chunk's 64 channels
    const int sq = tid & 3;
    const float* hsrc[3];
    size_t hpix[3];
    bool hlive[3], hin[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int hp = PT * j + (tid >> 2);
        hin[j] = hp < HP;
        const int wc = hp / HP2, hr = hp - wc * HP2;
        int w = w0 - 1 + wc;
        w = w < 0 ? w + W : (w >= W ? w - W : w);
        const int h = hr - 1;
        hlive[j] = hin[j] && h >= 0 && h < H;
        hpix[j] = (size_t)(b * W + w) * H + (hlive[j] ? h : 0);
        hsrc[j] = p.x + hpix[j] * Cin + sq * 16;
    }
    const int npass = (HP + PT - 1) / PT;                            // 2, or 3 (H = 2)
    const int swr = tid / TPR, shalf = tid % TPR;
    const int wrow = n0 + swr;
    const bf16_t* wptr = p.w + (size_t)(wrow < N ? wrow : 0) * 9 * Cin_pad + shalf * (CK / TPR);
    const int nck = Cin / CK;
    constexpr int D = 3;                            // weight stages in flight (one L2 latency = about three stage times)
    f32x4 xr[3][4];
    u32x4 wr[D][WV];
    auto fetch_x = [&](int cc) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < npass && hin[j]) {
                const float* src = hsrc[j] + cc * CK;
                if constexpr (FU) {                 // two sources: the chunk lies in one of them (C0 % 64 == 0)
                    const int c = cc * CK + sq * 16;
                    src = c < fC0 ? p.x + hpix[j] * fC0 + c : x1p + hpix[j] * (Cin - fC0) + (c - fC0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) xr[j][q] = reinterpret_cast<const f32x4*>(src)[q];
            }
    };
    // (FU) GroupNorm (+ SiLU) of halo pass j's staged values, in their registers.  For every chunk but the first it runs during the previous
    // chunk's last three taps, between their MFMAs (the values have been in flight since tap 2) -- as part of stash_x the whole workgroup
    // did VALU work between two barriers while the matrix pipe idled: + 9 us per 256x16 conv.
    auto xform = [&](int cc, int j) __attribute__((always_inline)) {
        if (j < npass && hin[j]) {
            const float2* co = sSc + cc * CK + sq * 16;
            const bool act = f.silu != 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 c_ = co[4 * q + e];
                    float z = xr[j][q][e] * c_.x + c_.y;
                    if (act) z *= tr_sigmoid(z);
                    xr[j][q][e] = z;
                }
        }
    };
    auto stash_x = [&](int cc, bool xformed) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < npass && hin[j]) {
                const float lv = hlive[j] ? 1.f : 0.f;
                bf16_t* dst = sXh + (PT * j + (tid >> 2)) * PITCH + sq * 16;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    f32x4 a = xr[j][2 * q], c = xr[j][2 * q + 1];
                    if constexpr (FU) {
                        if (in_gn && !xformed) {    // GroupNorm (+ SiLU) once per staged element; the halo's zero rows stay zeros (lv)
                            const float2* co = sSc + cc * CK + sq * 16 + 8 * q;
                            const bool act = f.silu != 0;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float2 c0_ = co[e], c1_ = co[4 + e];
                                float z0 = a[e] * c0_.x + c0_.y, z1 = c[e] * c1_.x + c1_.y;
                                if (act) { z0 *= tr_sigmoid(z0); z1 *= tr_sigmoid(z1); }
                                a[e] = z0; c[e] = z1;
                            }
                        }
                    }
                    u32x4 u;
                    u.x = rldm::pack_bf16x2(a.x * lv, a.y * lv); u.y = rldm::pack_bf16x2(a.z * lv, a.w * lv);
                    u.z = rldm::pack_bf16x2(c.x * lv, c.y * lv); u.w = rldm::pack_bf16x2(c.z * lv, c.w * lv);
                    *reinterpret_cast<u32x4*>(dst + 8 * q) = u;
                }
            }
    };
#define HALO_FETCH_W(SLOT, TAP, CC)                                                                      \
    {                                                                                                    \
        const bf16_t* src_ = wptr + (size_t)(TAP) * Cin_pad + (CC) * CK;                                 \
        _Pragma("unroll") for (int q = 0; q < WV; ++q) wr[SLOT][q] = reinterpret_cast<const u32x4*>(src_)[q]; \
    }
#define HALO_STASH_W(SLOT)                                                                               \
    _Pragma("unroll") for (int q = 0; q < WV; ++q)                                                       \
        *reinterpret_cast<u32x4*>(sW + swr * PITCH + shalf * (CK / TPR) + 8 * q) = wr[SLOT][q];
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    // this lane's pixel of the tile -> its row in the halo image
    constexpr int PG = PT / 32;                     // pixel groups of 32
    const int lp = (wave % PG) * 32 + l31;
    const int r0 = (lp / H + 1) * HP2 + (lp % H) + 1;
    const bf16_t* bx0 = sXh + r0 * PITCH + 8 * kg;
    const bf16_t* aw0 = sW + ((wave / PG) * (BN / 2) + l31) * PITCH + 8 * kg;
    const bf16_t* aw1 = aw0 + (NR == 2 ? 32 : 0) * PITCH;
    fetch_x(0);
    HALO_FETCH_W(0, 0, 0)
    HALO_FETCH_W(1, 1, 0)
    HALO_FETCH_W(2, 2, 0)
    if constexpr (FU) {                             // (behind the first loads; visible after the loop's first barrier)
        if (in_gn) tr_gn_coeffs(sSc, 0, Cin, f.cs0, f.cs1, fC0, Cin, b, f.groups, f.eps, W * H, f.gamma, f.beta);
        if (f.gs_out) tr_gn_coeffs_tile(sCe, BN, n0, f.gcs0, f.gcs1, f.G0, N, b, f.ggroups, f.geps, W * H, f.ggamma, f.gbeta);
    }
    for (int cc = 0; cc < nck; ++cc) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {         // (unrolled: the ring slot tap % D is a compile-time register set)
            __syncthreads();                        // everyone is done reading the previous stage (and, at tap 0, the halo tile)
            if (tap == 0) stash_x(cc, cc > 0);
            HALO_STASH_W(tap % D)
            __syncthreads();
            if (tap + D < 9) HALO_FETCH_W(tap % D, tap + D, cc)
            else if (cc + 1 < nck) HALO_FETCH_W(tap % D, tap + D - 9, cc + 1)
            if (tap == 2 && cc + 1 < nck) fetch_x(cc + 1);          // the next chunk's halo rides in registers for six taps
            const int toff = ((tap / 3) - 1) * HP2 + (tap % 3) - 1;
            const bf16_t* bx = bx0 + toff * PITCH;
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) {
                const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bx + 16 * ks);
                const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(aw0 + 16 * ks);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bv, acc0, 0, 0, 0);
                if (NR == 2) {
                    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(aw1 + 16 * ks);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bv, acc1, 0, 0, 0);
                }
            }
            if constexpr (FU) {
                if (in_gn && tap >= 6 && cc + 1 < nck) xform(cc + 1, tap - 6);
            }
        }
    }
    if constexpr (FU) {
        if (f.cs_out || f.gs_out) {
            float* tile = reinterpret_cast<float*>(hraw);
            __syncthreads();
            float* trow = tile + lp * (BN + 1) + (wave / PG) * (BN / 2);
#pragma unroll
            for (int h = 0; h < NR; ++h)
#pragma unroll
                for (int r = 0; r < 16; ++r) trow[32 * h + 8 * (r >> 2) + 4 * kg + (r & 3)] = h ? acc1[r] : acc0[r];
            __syncthreads();
            tr_tile_epilogue<BN, DET>(tile, sCol, sCe, p, f, px0, n0, b, true, true);
            return;
        }
    }
    const int px = px0 + lp;
    const int nb = n0 + (wave / PG) * (BN / 2);
    float* yrow = p.y + (size_t)px * N;
    const float* rrow = p.res ? p.res + (size_t)px * N : nullptr;
#pragma unroll
    for (int h = 0; h < NR; ++h)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
            const int ch = nb + 32 * h + 8 * (r >> 2) + 4 * kg;       // 4 consecutive channels per register quad (N % 4 == 0 here)
            if (ch >= N) continue;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = h ? acc1[r + e] : acc0[r + e];
            if (p.bias) { const f32x4 t = tr_load4(p.bias + ch); v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3]; }
            if (p.rowadd) { const float4 t = *reinterpret_cast<const float4*>(p.rowadd + (size_t)b * p.rowadd_ld + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            if (rrow) { const float4 t = *reinterpret_cast<const float4*>(rrow + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            if (p.accumulate) { const float4 t = *reinterpret_cast<const float4*>(yrow + ch); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            *reinterpret_cast<float4*>(yrow + ch) = make_float4(v[0], v[1], v[2], v[3]);
        }
#undef HALO_FETCH_W
#undef HALO_STASH_W
}

// ---- Linear layers on a handful of rows (time embedding MLP, the resnets' time_emb_proj: B <= 16 rows) -------------------------
// The MFMA conv kernel gives such a layer 4 workgroups that walk K serially (19 us for K = 512).  Here one wave owns one output
// feature: lanes stride over K in 16-byte pieces of the bf16 weight row, fp32 FMAs against the rows of x, butterfly at the end.
constexpr int LIN_MAXB = 16;
__global__ __launch_bounds__(256) void tr_linear_rows_kernel(const float* __restrict__ x, int ldx, const bf16_t* __restrict__ w, int Kp,
                                                             int K, const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                             int B, int N, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc[LIN_MAXB];
#pragma unroll
    for (int b = 0; b < LIN_MAXB; ++b) acc[b] = 0.f;
    const bf16_t* wr = w + (size_t)n * Kp;
    for (int k0 = lane * 8; k0 < K; k0 += 512) {
        const uint4 wv = *reinterpret_cast<const uint4*>(wr + k0);
        const float wf[8] = {rldm::bf16lo(wv.x), rldm::bf16hi(wv.x), rldm::bf16lo(wv.y), rldm::bf16hi(wv.y),
                             rldm::bf16lo(wv.z), rldm::bf16hi(wv.z), rldm::bf16lo(wv.w), rldm::bf16hi(wv.w)};
#pragma unroll
        for (int b = 0; b < LIN_MAXB; ++b) {
            if (b < B) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(x + (size_t)b * ldx + k0);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(x + (size_t)b * ldx + k0 + 4);
                acc[b] += a0[0] * wf[0] + a0[1] * wf[1] + a0[2] * wf[2] + a0[3] * wf[3] + a1[0] * wf[4] + a1[1] * wf[5] + a1[2] * wf[6] +
                          a1[3] * wf[7];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < LIN_MAXB; ++b) {
        if (b < B) {
            float v = acc[b];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            if (lane == 0) {
                float* dst = y + (size_t)b * ldy + n;
                v += bias ? bias[n] : 0.f;
                *dst = accumulate ? *dst + v : v;
            }
        }
    }
}

// the LDS-staged instances: [halo | CK 64 | CK 32][wide | narrow tile][plain | fused | fused deterministic]
typedef void (*ConvKernel)(const TrConv, const TrFuse);
const ConvKernel kConvKernels[3][2][3] = {
    {{tr_conv_halo_kernel<128>, tr_conv_halo_kernel<128, true>, tr_conv_halo_kernel<128, true, true>},
     {tr_conv_halo_kernel<64>, tr_conv_halo_kernel<64, true>, tr_conv_halo_kernel<64, true, true>}},
    {{tr_conv_lds_kernel<64, 128>, tr_conv_lds_kernel<64, 128, true>, tr_conv_lds_kernel<64, 128, true, true>},
     {tr_conv_lds_kernel<64, 64>, tr_conv_lds_kernel<64, 64, true>, tr_conv_lds_kernel<64, 64, true, true>}},
    {{tr_conv_lds_kernel<32, 128>, tr_conv_lds_kernel<32, 128, true>, tr_conv_lds_kernel<32, 128, true, true>},
     {tr_conv_lds_kernel<32, 64>, tr_conv_lds_kernel<32, 64, true>, tr_conv_lds_kernel<32, 64, true, true>}}};

}  // namespace

bool rldm::train::conv_desc_split(const rldm_train_conv_desc* d, rldm_train_conv_desc* plain, int* pad) {
    *plain = *d;
    *pad = (d->mode & RLDM_TRAIN_PAD_END) ? 1 : 0;
    plain->mode = d->mode & ~RLDM_TRAIN_PAD_END;
    if (!((d->taps == 1 || d->taps == 9) && (d->stride == 1 || d->stride == 2) && plain->mode >= 0 && plain->mode <= 2)) return false;
    return !*pad || (d->taps == 9 && ((d->stride == 2 && plain->mode == 0) || (d->stride == 1 && plain->mode == 2)));
}

extern "C" {

// launch shape of the LDS-staged conv: narrow (64-channel) tile? how many K splits?  (shared by rldm_train_conv and
// rldm_train_conv_splits, which lets the host hand out pre-zeroed outputs to the split launches)
static void conv_lds_plan(int P, int N, int Cin, int taps, bool* narrow_out, int* ksplit_out) {
    const long long gx = (P + 63) / 64;
    long long gy = (N + 127) / 128;
    // 128-channel tiles stage the pixel operand half as often; 64-channel tiles double the workgroups in flight, which
    // is what hides a stage's load latency when the launch has fewer than ~2 workgroups per CU (3x3 levels 1-3: 10-20 %
    // faster; the 512-workgroup level 0 and the two-stage 1x1 convs are faster with the wide tile)
    const bool narrow = taps == 9 && gx * gy < 512;   // (measured per level)
    if (narrow) gy = (N + 63) / 64;
    // split K when the launch cannot fill the chip (see the kernel): aim at >= kTarget workgroups, >= kMinStages stages each (the
    // split width is on a plateau from 128 to 512 target workgroups; more splits lose 1 - 8 %)
    constexpr int kTarget = 512, kMinStages = 3;
    const int niter = taps * (Cin / (Cin % 64 == 0 ? 64 : 32));
    const long long wgs = gx * gy;
    // (deterministic mode: never split -- a workgroup contracts all of K in stage order)
    const int ksplit = wgs > 192 || deterministic() ? 1 : (int)std::min<long long>((kTarget + wgs - 1) / wgs, niter / kMinStages);
    *narrow_out = narrow;
    *ksplit_out = std::max(1, std::min(ksplit, niter));
}

int rldm_train_conv_splits(const rldm_train_conv_desc* d0, int rowadd_ld) {
    rldm_train_conv_desc plain;
    int pad;
    if (!d0 || d0->stride < 1 || !conv_desc_split(d0, &plain, &pad)) return 1;
    const rldm_train_conv_desc* d = &plain;
    const int sh = d->mode ? 1 : 0;
    const int P = d->B * ((d->Win << sh) / d->stride) * ((d->Hin << sh) / d->stride);
    if (!(P >= 64 && (rowadd_ld & 3) == 0 && d->Cin % 32 == 0)) return 1;
    bool narrow;
    int ksplit;
    conv_lds_plan(P, d->N, d->Cin, d->taps, &narrow, &ksplit);
    return ksplit;
}

// can the fused conv kernels run this launch?  (LDS-staged kernels; tiles inside one image; chunks inside one source)
static bool conv_fuse_ok(const rldm_train_conv_desc* d, const rldm_train_fuse* fu, int rowadd_ld) {
    const int sh = d->mode ? 1 : 0;
    const int Wout = (d->Win << sh) / d->stride, Hout = (d->Hin << sh) / d->stride;
    const int P = d->B * Wout * Hout, CK = d->Cin % 64 == 0 ? 64 : 32;
    if (!(P >= 64 && (rowadd_ld & 3) == 0 && d->Cin % 32 == 0 && (Wout * Hout) % 64 == 0)) return false;
    if (fu->x1 && (fu->C0 <= 0 || fu->C0 >= d->Cin || fu->C0 % CK != 0 || (d->Cin - fu->C0) % 4 != 0 || fu->C0 % 4 != 0)) return false;
    if (fu->cs0 && (d->Cin > 768 || fu->groups < 1 || fu->groups > 64 || d->Cin % fu->groups != 0 || !fu->gamma || !fu->beta || (fu->x1 && !fu->cs1))) return false;
    if (fu->cs_out && fu->gs_out) return false;
    if ((fu->cs_out || fu->gs_out) && d->N % 4 != 0) return false;          // (the tile epilogue works on channel quads)
    if (fu->gs_out) {
        if (!fu->g0 || !fu->gcs0 || !fu->ggamma || !fu->gbeta || fu->ggroups < 1 || d->N % fu->ggroups != 0) return false;
        if (fu->g1 && (!fu->gcs1 || fu->G0 <= 0 || fu->G0 >= d->N || fu->G0 % 4 != 0)) return false;
    }
    return true;
}

int rldm_train_conv_fused_ok(const rldm_train_conv_desc* d, const rldm_train_fuse* fu, int rowadd_ld) {
    // (no fused instance reads the end-only padding: RLDM_TRAIN_PAD_END is refused like every mode past 2)
    return d && fu && d->stride >= 1 && d->mode >= 0 && d->mode <= 2 && conv_fuse_ok(d, fu, rowadd_ld) ? 1 : 0;
}

static int train_conv_impl(const rldm_train_conv_desc* d0, const rldm_train_fuse* fu, const float* x, const void* w_packed, const float* bias,
                           const float* rowadd, int rowadd_ld, const float* res, float* y, int accumulate, void* stream) {
    RLDM_REQUIRE(d0 && x && w_packed && y, "null argument");
    rldm_train_conv_desc plain;
    int pad;
    RLDM_REQUIRE(conv_desc_split(d0, &plain, &pad), "bad conv desc");
    const rldm_train_conv_desc* d = &plain;
    RLDM_REQUIRE(d->B > 0 && d->Win > 0 && d->Hin > 0 && d->Cin > 0 && d->N > 0, "bad shape");
    TrConv p;
    p.x = x; p.w = static_cast<const bf16_t*>(w_packed); p.bias = bias; p.rowadd = rowadd; p.res = res; p.y = y;
    p.B = d->B; p.Win = d->Win; p.Hin = d->Hin; p.Cin = d->Cin; p.Cin_pad = (d->Cin + 15) / 16 * 16;
    const int sh = d->mode ? 1 : 0;
    p.Wout = (d->Win << sh) / d->stride; p.Hout = (d->Hin << sh) / d->stride;
    RLDM_REQUIRE(p.Wout > 0 && p.Hout > 0, "empty output");
    p.N = d->N; p.taps = d->taps; p.stride = d->stride; p.mode = d->mode; p.rowadd_ld = rowadd_ld; p.accumulate = accumulate;
    p.shift = conv_desc_shift(d, pad);
    const int P = p.B * p.Wout * p.Hout;
    dim3 grid((P + 63) / 64, (p.N + 127) / 128);
    const bool aligned = (rowadd_ld & 3) == 0;         // (vector epilogue reads the per-sample row 16 bytes at a time)
    const bool lds = P >= 64 && aligned;               // Linear layers on a handful of rows: the direct kernel
    hipStream_t st = (hipStream_t)stream;
    TrFuse f = to_device_fuse(fu, p.Cin, p.N);
    if (lds && p.Cin % 32 == 0) {
        bool narrow;
        int ksplit;
        conv_lds_plan(P, p.N, p.Cin, p.taps, &narrow, &ksplit);
        if (narrow) grid.y = (p.N + 63) / 64;
        if (ksplit > 1) {
            if (!accumulate && launch_zero(y, (size_t)P * p.N, st)) return 1;     // (a kernel, not a memset node: see tr_zero_kernel)
            grid.z = ksplit;
            // (arrival counters of the fused split-K launches: every launch leaves them zeroed)
            if (fu && (f.cs_out || f.gs_out) &&
                tr_scratch(kFuseTickets, (size_t)grid.x * grid.y * sizeof(unsigned), 16384 * sizeof(unsigned), true, st,
                           reinterpret_cast<void**>(&f.tickets)))
                return 1;
        } else if (fu && (f.cs_out || f.gs_out)) {
            // (deterministic mode: a caller that asked rldm_train_conv_splits with the mode off may hand in a zeroed y; it is written)
            RLDM_REQUIRE(!accumulate || deterministic(), "rldm_train_conv_fused: the fused epilogue writes y (no accumulation)");
            p.accumulate = 0;
        }
        // deterministic mode: the epilogue leaves one partial row per 64-pixel tile, folded in tile order behind the launch
        const bool det_sums = deterministic() && fu && (f.cs_out || f.gs_out);
        if (det_sums && det_partials((size_t)grid.x * p.N * 2 * sizeof(float), st, reinterpret_cast<void**>(&f.part))) return 1;
        {                                           // the previous weight gradient's reduction rides on this launch
            const int planes = attach_reduce(f, st, grid.x, grid.y, grid.z);
            if (planes < 0) return 1;
            grid.z += planes;
        }
        const int H = p.Hout;
        const bool halo = ksplit == 1 && p.taps == 9 && p.stride == 1 && p.mode == 0 && p.Cin % 64 == 0 && p.N % 4 == 0 &&
                          H >= 2 && H <= 32 && (H & (H - 1)) == 0 && (p.Wout * H) % 64 == 0 && p.Wout % (64 / H) == 0 && p.Wout >= 64 / H + 2;
        kConvKernels[halo ? 0 : (p.Cin % 64 == 0 ? 1 : 2)][narrow ? 1 : 0][det_sums ? 2 : (fu ? 1 : 0)]<<<grid, 256, 0, st>>>(p, f);
        if (det_sums) {
            TR_LAUNCH_CHECK();
            const int tiles = p.Wout * p.Hout / 64;     // per image (conv_fuse_ok: a multiple of 64 pixels)
            if (launch_fold_rows(f.part, p.B, tiles, 2 * p.N, f.gs_out ? f.gs_out : f.cs_out, 2 * p.N, 1, st)) return 1;
        }
    } else {
        RLDM_REQUIRE(!fu, "rldm_train_conv_fused: not an LDS-staged shape");
        if (flush_reduce()) return 1;
        if (p.Cin % 16 == 0) tr_conv_kernel<true><<<grid, 256, 0, st>>>(p);
        else tr_conv_kernel<false><<<grid, 256, 0, st>>>(p);
    }
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_train_conv(const rldm_train_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* rowadd,
                    int rowadd_ld, const float* res, float* y, int accumulate, void* stream) {
    return train_conv_impl(d, nullptr, x, w_packed, bias, rowadd, rowadd_ld, res, y, accumulate, stream);
}

int rldm_train_conv_fused(const rldm_train_conv_desc* d, const rldm_train_fuse* fu, const float* x, const void* w_packed, const float* bias,
                          const float* rowadd, int rowadd_ld, const float* res, float* y, int prezeroed, void* stream) {
    RLDM_REQUIRE(d && fu, "null argument");
    RLDM_REQUIRE(rldm_train_conv_fused_ok(d, fu, rowadd_ld), "rldm_train_conv_fused: shape not supported (ask rldm_train_conv_fused_ok)");
    return train_conv_impl(d, fu, x, w_packed, bias, rowadd, rowadd_ld, res, y, prezeroed, stream);
}

int rldm_train_linear_rows(const float* x, int ldx, const void* w_packed, int K, const float* bias, float* y, int ldy, int B, int N,
                           int accumulate, void* stream) {
    RLDM_REQUIRE(x && w_packed && y, "null argument");
    RLDM_REQUIRE(B >= 1 && B <= LIN_MAXB && K % 8 == 0 && ldx % 4 == 0, "rows <= 16, K a multiple of 8");
    const int Kp = (K + 15) / 16 * 16;
    tr_linear_rows_kernel<<<(N + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, ldx, static_cast<const bf16_t*>(w_packed), Kp, K, bias, y, ldy, B,
                                                                       N, accumulate);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
