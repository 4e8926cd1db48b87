// The phase record of the persistent trunk launch (trunk.hip): the format, the plan builder's encoders (plan.hip) and the kernel's
// decoders, side by side -- a field added to one must be added to the other.
#pragma once
#include "kernels.h"

#include <cstdint>
#include <cstring>

namespace rldm {

// A phase record is 64 dwords: ONE vector load per wave (lane l holds word l), requested a phase ahead, and v_readlane puts the
// fields into SGPRs -- the place the kernel-argument copy of a stand-alone launch lives in.
enum TrunkWord {
    TW_X0 = 0, TW_R0 = 2, TW_R1 = 4, TW_WPK = 6, TW_BIAS = 8, TW_Y = 10, TW_YSTATS = 12, TW_RES = 14,    // 64-bit pointers
    TW_R0C = 16, TW_R1C, TW_WIN, TW_HIN, TW_WOUT, TW_HOUT, TW_TW, TW_TH, TW_COLB, TW_THSHIFT, TW_N, TW_YLD, TW_NVIEWS,
    TW_KIND, TW_G, TW_NMINE, TW_TEMBOFF,
    TW_NV0 = 34,            // 2 views x 11 words: y (2), gamma (2), beta (2), ld, cpg_shift, inv_n, eps, silu
    TW_NVSTRIDE = 11,
    // phases of a MULTI-TILE cluster (kind >= 8: an image is several 64-pixel tiles x 64-channel tiles; no views) keep the
    // consumer-side GroupNorm of their input in the words the views would occupy
    TW_ST0 = 34, TW_GAMMA = 36, TW_BETA = 38,                   // 64-bit pointers
    TW_P0 = 40, TW_GROUPS, TW_MAGIC_CPG, TW_INVN, TW_EPS, TW_SILU, TW_TILES_H, TW_TILES_IMG,
    // conv_stream phases (kind 15: the full-resolution levels as clusters of 16 or 32 pixel tiles)
    TW_X1 = 48, TW_ST1 = 50,                                    // 64-bit pointers
    TW_C0 = 52, TW_C1, TW_P1, TW_MAGIC_THV, TW_UP,
    TW_SUB,                 // conv_stream phases of variant 4, a TrunkStreamForm (kernels.h): TSF_SUB = the sub-pixel form of nearest x2 + 3x3 (rank =
                            // input tile * 4 + parity, 128 output channels), TSF_FULLH = tiles as tall as the image
    TW_WBYTES = 58,         // bytes of the phase's packed weights (TW_WPK ...): what the PREVIOUS phase touches, one dword per 128-byte line,
                            // so that they wait in the XCD's L2 (round 5: trunk_warm_next; 0: nothing to warm)
    TW_WORDS = 64
};
// phase kinds: 0..2 / 4..6 image-owning conv_small tiles (64 / 32 pixels), 3 attention over a pre-normalised x,
// 9..11 3x3 conv over 256 / 384 / 512 channels on 64-pixel x 64-channel tiles of a multi-tile image (8: 128 channels, not instantiated), 12 its 1x1 over 256,
// 13 attention with the GroupNorm fold inside (two query tiles per wave)
// 14 GroupNorm (+ SiLU) of a concatenated input as a phase of its own (norm.hip's gn_apply_kernel; record: x0 / x1 in TW_X0 / TW_R0,
// their channels in TW_R0C / TW_R1C, statistics in TW_ST0 / TW_RES with TW_P0 / TW_TILES_H partials, pixels per image in TW_WIN)
// (round 5) 16..18: the image-owning 64-pixel kinds 0..2 on 16-channel tiles (conv_small_body's H16 instances)
enum TrunkKind { TK_H16 = 16, TK_ATTN = 3, TK_CL_3x3_128 = 8, TK_CL_3x3_256, TK_CL_3x3_384, TK_CL_3x3_512, TK_CL_1x1_256, TK_ATTN_FOLD, TK_GN_APPLY, TK_STREAM };
struct TrunkPhase {
    unsigned w[TW_WORDS];
};

// ---- the plan builder's side: a filled parameter block -> record.  Pointers as two words, floats by their bits; every word a function
// does not name is 0.  The caller adds what belongs to the segment, not to the layer: TW_G, TW_NMINE, TW_WBYTES.
inline void put64(TrunkPhase& ph, int at, const void* ptr) {
    const unsigned long long u = (unsigned long long)(uintptr_t)ptr;
    ph.w[at] = (unsigned)u;
    ph.w[at + 1] = (unsigned)(u >> 32);
}
inline void putf(TrunkPhase& ph, int at, float f) { memcpy(&ph.w[at], &f, 4); }
// the consumer-side GroupNorm of a phase's input (words 34 to 47 in their second meaning)
inline void put_consumer_gn(TrunkPhase& ph, const float2* st, const float* gamma, const float* beta, int P, int groups, int magic_cpg,
                            float inv_n, float eps) {
    put64(ph, TW_ST0, st); put64(ph, TW_GAMMA, gamma); put64(ph, TW_BETA, beta);
    ph.w[TW_P0] = P; ph.w[TW_GROUPS] = groups; ph.w[TW_MAGIC_CPG] = magic_cpg;
    putf(ph, TW_INVN, inv_n); putf(ph, TW_EPS, eps);
}
// A conv phase (unpack_phase; consumer_gn: unpack_cluster_phase / unpack_stream_phase).  consumer_gn = false: an image-owning tile, words
// 34.. carry the normalised views it writes (at most two); true: a tile of a multi-tile cluster or a conv_stream tile, they carry the
// GroupNorm of its input, and the words behind them the second tensor of a concatenation and the tile grid.
inline TrunkPhase trunk_conv_phase(const ConvParams& p, int kind, bool consumer_gn, int temb_off) {
    TrunkPhase ph;
    memset(&ph, 0, sizeof(ph));
    put64(ph, TW_X0, p.x0); put64(ph, TW_R0, p.r0); put64(ph, TW_R1, p.r1); put64(ph, TW_WPK, p.wpk); put64(ph, TW_BIAS, p.bias);
    put64(ph, TW_Y, p.y); put64(ph, TW_YSTATS, p.y_stats); put64(ph, TW_RES, p.res);
    ph.w[TW_R0C] = p.R0; ph.w[TW_R1C] = p.R1; ph.w[TW_WIN] = p.Win; ph.w[TW_HIN] = p.Hin; ph.w[TW_WOUT] = p.Wout;
    ph.w[TW_HOUT] = p.Hout; ph.w[TW_TW] = p.TW; ph.w[TW_TH] = p.TH; ph.w[TW_COLB] = p.colb; ph.w[TW_THSHIFT] = p.th_shift;
    ph.w[TW_N] = p.N; ph.w[TW_YLD] = p.y_ld; ph.w[TW_NVIEWS] = p.nviews;
    ph.w[TW_KIND] = kind; ph.w[TW_TEMBOFF] = (unsigned)temb_off;
    if (consumer_gn) {
        put_consumer_gn(ph, p.st0, p.gn_gamma, p.gn_beta, p.P0, p.gn_groups, p.magic_cpg, p.gn_inv_n, p.gn_eps);
        ph.w[TW_SILU] = p.silu; ph.w[TW_TILES_H] = p.tiles_h; ph.w[TW_TILES_IMG] = p.tiles_img;
        put64(ph, TW_X1, p.x1); put64(ph, TW_ST1, p.st1);
        ph.w[TW_C0] = p.C0; ph.w[TW_C1] = p.C1; ph.w[TW_P1] = p.P1;
        ph.w[TW_MAGIC_THV] = p.magic_thv; ph.w[TW_UP] = p.up;
        if (kind == TK_STREAM) ph.w[TW_SUB] = stream_inst(p).trunk;          // (conv_stream's sub-pixel / full-height instances)
    } else {
        for (int v = 0; v < 2 && v < p.nviews; ++v) {
            const int at = TW_NV0 + v * TW_NVSTRIDE;
            put64(ph, at, p.nv[v].y); put64(ph, at + 2, p.nv[v].gamma); put64(ph, at + 4, p.nv[v].beta);
            ph.w[at + 6] = p.nv[v].ld; ph.w[at + 7] = p.nv[v].cpg_shift;
            putf(ph, at + 8, p.nv[v].inv_n); putf(ph, at + 9, p.nv[v].eps);
            ph.w[at + 10] = p.nv[v].silu;
        }
    }
    return ph;
}
// The attention core of a block (decoded as a conv phase, then read by trunk_kernel's attention branch): x pre-normalised (TK_ATTN), or raw
// with the producer's statistics in the consumer-side GroupNorm words (ap.st set: TK_ATTN_FOLD, multi-tile clusters).
inline TrunkPhase trunk_attention_phase(const AttnQkvParams& ap) {
    TrunkPhase ph;
    memset(&ph, 0, sizeof(ph));
    put64(ph, TW_X0, ap.x); put64(ph, TW_WPK, ap.wfrag); put64(ph, TW_BIAS, ap.bias); put64(ph, TW_Y, ap.out);
    ph.w[TW_WIN] = ap.L; ph.w[TW_N] = ap.C;
    ph.w[TW_KIND] = ap.st ? TK_ATTN_FOLD : TK_ATTN; ph.w[TW_TEMBOFF] = (unsigned)-1;
    if (ap.st) put_consumer_gn(ph, ap.st, ap.gamma, ap.beta, ap.P, ap.groups, ap.magic_cpg, ap.inv_n, ap.eps);
    return ph;
}
// GroupNorm (+ SiLU) of a concatenated input as a phase (kind TK_GN_APPLY, decoded by unpack_cluster_phase; the field-to-word map is in the
// list of kinds above; g.inv_n filled by the caller)
inline TrunkPhase trunk_gn_apply_phase(const GnApplyParams& g) {
    TrunkPhase ph;
    memset(&ph, 0, sizeof(ph));
    put64(ph, TW_X0, g.x0); put64(ph, TW_R0, g.x1); put64(ph, TW_RES, g.st1); put64(ph, TW_Y, g.y);
    ph.w[TW_R0C] = g.C0; ph.w[TW_R1C] = g.C1; ph.w[TW_TILES_H] = g.P1; ph.w[TW_WIN] = g.npix;
    put_consumer_gn(ph, g.st0, g.gamma, g.beta, g.P0, g.groups, 0, g.inv_n, g.eps);
    ph.w[TW_SILU] = g.silu;
    ph.w[TW_KIND] = TK_GN_APPLY; ph.w[TW_TEMBOFF] = (unsigned)-1;
    return ph;
}

// ---- the kernel's side (trunk.hip): every wave loads the record with ONE instruction (lane l = word l) a phase ahead,
// and v_readlane moves the fields into SGPRs -- where the kernel-argument copy of a stand-alone launch lives.  (Reading the record
// field by field would be ~60 dependent VECTOR loads per phase: the launch also writes device memory, so the compiler may not use
// scalar loads for it.)
__device__ __forceinline__ unsigned rl(unsigned rec, int word) { return (unsigned)__builtin_amdgcn_readlane((int)rec, word); }
// The pointer is built as a GLOBAL-address-space pointer and only then converted to the generic type the bodies take: the compiler
// then proves every access through it global and emits global_load / global_store.  Built from an integer alone it is a FLAT pointer:
// every load and store of every phase became a flat_* instruction, which counts on lgkmcnt as well as vmcnt -- each LDS wait of a K
// loop then also waited for the whole weight ring in flight, i.e. the ring was no ring (round 3: the "open question" of DESIGN.md 3.7,
// a 128x8 phase's K loop 16.3 k cycles against 12.8 k in the stand-alone launch; tools/l1_probe.sh).
template <class T> __device__ __forceinline__ T* rl_ptr(unsigned rec, int word) {
    typedef __attribute__((address_space(1))) T* global_ptr_t;
    return (T*)(global_ptr_t)(((unsigned long long)rl(rec, word + 1) << 32) | rl(rec, word));
}
__device__ __forceinline__ void unpack_phase(ConvParams& q, unsigned rec) {
    q.x0 = rl_ptr<const bf16_t>(rec, TW_X0);
    q.r0 = rl_ptr<const bf16_t>(rec, TW_R0);
    q.r1 = rl_ptr<const bf16_t>(rec, TW_R1);
    q.wpk = rl_ptr<const bf16_t>(rec, TW_WPK);
    q.bias = rl_ptr<const float>(rec, TW_BIAS);
    q.y = rl_ptr<bf16_t>(rec, TW_Y);
    q.y_stats = rl_ptr<float2>(rec, TW_YSTATS);
    q.res = rl_ptr<const bf16_t>(rec, TW_RES);
    q.R0 = (int)rl(rec, TW_R0C); q.R1 = (int)rl(rec, TW_R1C);
    q.Win = (int)rl(rec, TW_WIN); q.Hin = (int)rl(rec, TW_HIN); q.Wout = (int)rl(rec, TW_WOUT); q.Hout = (int)rl(rec, TW_HOUT);
    q.TW = (int)rl(rec, TW_TW); q.TH = (int)rl(rec, TW_TH); q.colb = (int)rl(rec, TW_COLB); q.th_shift = (int)rl(rec, TW_THSHIFT);
    q.N = (int)rl(rec, TW_N); q.y_ld = (int)rl(rec, TW_YLD); q.nviews = (int)rl(rec, TW_NVIEWS);
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int at = TW_NV0 + v * TW_NVSTRIDE;
        q.nv[v].y = rl_ptr<bf16_t>(rec, at);
        q.nv[v].gamma = rl_ptr<const float>(rec, at + 2);
        q.nv[v].beta = rl_ptr<const float>(rec, at + 4);
        q.nv[v].ld = (int)rl(rec, at + 6);
        q.nv[v].cpg_shift = (int)rl(rec, at + 7);
        q.nv[v].inv_n = __uint_as_float(rl(rec, at + 8));
        q.nv[v].eps = __uint_as_float(rl(rec, at + 9));
        q.nv[v].silu = (int)rl(rec, at + 10);
    }
    q.nv[2] = q.nv[1];                          // (trunk phases write at most two copies)
    // what a trunk phase never has / what its tile implies
    q.x1 = nullptr; q.C0 = 0; q.C1 = 0; q.st0 = nullptr; q.st1 = nullptr; q.P0 = 0; q.P1 = 0; q.temb = nullptr; q.step_ptr = nullptr;
    q.ts = nullptr; q.up = 1; q.stride = 1; q.tiles_h = 1; q.tiles_img = 1; q.dbg = 0; q.silu = 0; q.B = 0;
}
// a phase of a multi-tile cluster (kind >= 8): no views; the words they would occupy carry the consumer-side GroupNorm of the input
__device__ __forceinline__ void unpack_cluster_phase(ConvParams& q, unsigned rec) {
    unpack_phase(q, rec);
    q.nviews = 0;
    q.st0 = rl_ptr<const float2>(rec, TW_ST0);
    q.gn_gamma = rl_ptr<const float>(rec, TW_GAMMA);
    q.gn_beta = rl_ptr<const float>(rec, TW_BETA);
    q.P0 = (int)rl(rec, TW_P0);
    q.gn_groups = (int)rl(rec, TW_GROUPS);
    q.magic_cpg = (int)rl(rec, TW_MAGIC_CPG);
    q.gn_inv_n = __uint_as_float(rl(rec, TW_INVN));
    q.gn_eps = __uint_as_float(rl(rec, TW_EPS));
    q.silu = (int)rl(rec, TW_SILU);
    q.tiles_h = (int)rl(rec, TW_TILES_H);
    q.tiles_img = (int)rl(rec, TW_TILES_IMG);
    q.up = max((int)rl(rec, TW_UP), 1);         // (nearest x2 folded into the staging of an up-sampler's conv)
    // (round 4) a concatenated input normalised by the phase itself: second tensor, its statistics, the split (C1 == 0: one tensor)
    q.x1 = rl_ptr<const bf16_t>(rec, TW_X1);
    q.st1 = rl_ptr<const float2>(rec, TW_ST1);
    q.C0 = (int)rl(rec, TW_C0); q.C1 = (int)rl(rec, TW_C1); q.P1 = (int)rl(rec, TW_P1);
}
// a conv_stream phase (kind TK_STREAM): the cluster words + the halo divisor
__device__ __forceinline__ void unpack_stream_phase(ConvParams& q, unsigned rec) {
    unpack_cluster_phase(q, rec);
    q.magic_thv = (int)rl(rec, TW_MAGIC_THV);
}

}  // namespace rldm
