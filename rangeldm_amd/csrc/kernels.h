// Kernel parameter blocks and launchers of librangeldm_hip (gfx950).  Activations: bf16 channels-last [B][W][H][C].
#pragma once
#include "common.h"

namespace rldm {

// ---------------------------------------------------------------------------------------------------------------
// Fused circular implicit-GEMM convolution (conv_igemm.hip)
//   y = conv_k( pad( silu?( GN?( cat[x0, x1] ) ) ) ) + bias (+ temb[row]) (+ res)
// geometry: virtual input v(w', h') = x(w'/up, h'/up) of size (Win*up, Hin*up); output pixel (w, h) reads
//   v(wrap(w*stride + i - pad_lo), h*stride + j - pad_lo) for taps i (azimuth), j (beams); h out of range -> 0.
// Reference arithmetic: ldm/utils.py:40-55,107-116; vae/sgm/modules/diffusionmodules/model.py:93-125,164-172.
// ---------------------------------------------------------------------------------------------------------------
// A normalised (+ activated) copy of a conv's output, written by the PRODUCER's epilogue for one consuming GroupNorm
// (conv_small.hip, tiles that own a whole image: the statistics of its 32 channels are complete inside the workgroup).
// y = silu?( gamma * (x - mean_g) * rstd_g + beta ) on the bf16-rounded output, stored at channel offset of the consumer's
// (possibly concatenated) input tensor.
struct NormView {
    bf16_t* y;              // consumer's pre-activated input [B][W][H][ld], already offset to this producer's first channel
    const float* gamma;     // consumer's GroupNorm affine, offset the same way
    const float* beta;
    int ld;
    int cpg_shift;          // log2(channels per group) of the CONSUMER's norm (<= 5: a 32-channel tile holds whole groups)
    float inv_n;            // 1 / (pixels per image * channels per group)
    float eps;
    int silu;
};

// The scheduler step fused into conv_out's fp32 NCHW epilogue (conv_igemm.hip): the thread that produces eps[i] also holds the
// index of x[i], so x_prev[i] = step(x[i], eps[i], noise[i]) costs one more load and store instead of a launch of its own
// (DDIMScheduler.step / DDPMScheduler.step; same arithmetic as sched_step_kernel).
// One scheduler step without its noise term.  mode = (ddpm ? 1 : 0) | prediction << 1 | (multistep ? kSchedMultistep : 0),
// prediction 0 epsilon | 1 v_prediction | 2 sample
// (diffusers DDIMScheduler.step / DDPMScheduler.step [3P]; the `prediction_type` branches ahead of the update).
// c0 = sqrt(alpha_prod_t), c1 = sqrt(beta_prod_t); DDIM: c2 = sqrt(alpha_prod_prev), c3 = direction coefficient (multiplies the
// predicted epsilon); DDPM: c2 / c3 = the posterior mean's coefficients of x0 / x_t.  The epsilon branch is the expression the
// kernels have always used (bit-identical).  x0_out receives the predicted x0 (the multistep solver's history).
// Multistep mode (DPM-Solver++(2M), diffusers DPMSolverMultistepScheduler): the DDPM update with c0 = alpha_i, c1 = sigma_i,
// c2 / c3 = the coefficients of x0 / x_t, and the third term c4 * x0 of the PREVIOUS step read from the history buffer that sits in
// the noise slot (step stride 0); the same thread then stores this step's x0 there.  The buffer is not read when c4 == 0.
// The step is inlined into four kernels (sched_step_kernel, sched_guided_step_kernel, the fp32-NCHW epilogue of conv_igemm.hip and
// conv_o4_kernel), and a sampler may run any of them for the same step, so its roundings are stated here, once, with contraction off:
// which products are fused into an fma and which are rounded on their own does not depend on the code around the inlining site
// (left to the compiler, the generic conv's epilogue rounded the v_prediction products differently from the other three).  The
// sequence is the one sched_step_kernel has always compiled to; tests/test_sched_tail_exact.py holds the sites bit-equal.
// nz: the noise (multistep mode: the previous x0) of this element, read by the caller only when use_noise (c4 != 0).
constexpr int kSchedMultistep = 8;
__device__ __forceinline__ float sched_prev(const int mode, const float c0, const float c1, const float c2, const float c3, const float c4,
                                            const float x, const float e, const float nz, const bool use_noise, float& x0_out) {
#pragma clang fp contract(off)
    const int pred = (mode >> 1) & 3;
    float x0, pe;
    if (pred == 0) {
        x0 = __builtin_fmaf(-c1, e, x) / c0;
        pe = e;
    } else if (pred == 1) {
        const float c1e = c1 * e, c0e = c0 * e;
        x0 = __builtin_fmaf(c0, x, -c1e);
        pe = __builtin_fmaf(c1, x, c0e);
    } else {
        x0 = e;
        pe = __builtin_fmaf(-c0, e, x) / c1;
    }
    x0_out = x0;
    const float a = c2 * x0;
    const float b = c3 * ((mode & 1) == 0 ? pe : x);
    float u = a + b;
    if (use_noise) u = __builtin_fmaf(c4, nz, u);
    return u;
}
// the x0 history of a multistep step (the noise slot, written after it was read), or null
__device__ __forceinline__ float* sched_history(const int mode, const float* slot) {
    return (mode & kSchedMultistep) ? const_cast<float*>(slot) : nullptr;
}

struct SchedFuse {
    const float* coef_table;  // device [steps][5]; null: not fused
    const int* step_ptr;
    const float* x;
    const float* noise;       // [steps][noise_step_stride] or null; multistep mode: the x0 history (stride 0, rewritten)
    long long noise_step_stride;
    float* x_prev;
    int mode;                 // 0 ddim, 1 ddpm; | prediction type << 1 | kSchedMultistep (sched_prev)
    // the NEXT step's conv_in input (pack_input's bf16 [B][W][H][pack_ld] tensor): the thread that holds x_prev[i] stores its bf16 image
    // too, so a step's first launch is conv_in instead of a pack launch (the pos-encoding / condition channels never change); or null
    bf16_t* pack;
    int pack_ld;
};

struct ConvParams {
    // main phase: TAPS taps per CK-channel chunk over cat[x0, x1], GroupNorm (+SiLU) applied on the way into LDS
    const bf16_t* x0;
    const bf16_t* x1;       // second tensor of a channel concat (may be null)
    int C0, C1;             // channels of x0 / x1; C0 and C0 + C1 are multiples of the kernel's CK
    // residual phase: one centre tap per chunk over cat[r0, r1] (raw, at OUTPUT resolution) with the 1x1 shortcut
    // weights (or an identity) appended to the weight stream; R0 + R1 == 0: none
    const bf16_t* r0;
    const bf16_t* r1;
    int R0, R1;
    int B, Win, Hin;
    int up;                 // 1 | 2 (nearest upsample folded into indexing)
    int stride;             // 1 | 2
    int pad_lo;             // 1: symmetric pad 1, 0: end-only pad (or 1x1)
    int Wout, Hout;
    int TW, TH;             // output-pixel tile handled by one block (TW*TH <= BM)
    int colb;               // halo column pitch in bytes (conv_halo_col_bytes)
    int tiles_h, tiles_img; // Hout / TH, (Wout / TW) * tiles_h
    int th_shift;           // log2(TH) (TH is a power of two)
    int magic_thv;          // ceil(2^20 / halo rows): slot / THv == (slot * magic) >> 20
    int magic_cpg;          // ceil(2^20 / channels per group)
    // GroupNorm prologue (null st0 -> none): per-channel partial (sum, sumsq) [B][P][C] written by the producers of x0/x1
    const float2* st0;
    const float2* st1;
    int P0, P1;
    int gn_groups;
    const float* gn_gamma;
    const float* gn_beta;
    float gn_eps;
    int silu;
    // weights: bf16, packed [ntile_n][Cin/CK * taps + (R0+R1)/CK][BN][CK + 8 pad]
    const bf16_t* wpk;
    int N;                  // real output channels
    int ntile_n;
    const float* bias;      // padded to ntile_n * BN
    // accumulator init: bias + temb row
    const float* temb;      // null or [rows][temb_ld], row = step*rows_per_step + (per_sample ? b : 0)
    int temb_ld;
    const int* step_ptr;    // device int (null -> 0)
    int temb_rows_per_step;
    int temb_per_sample;
    // outputs
    bf16_t* y;              // bf16 channels-last [B][Wout][Hout][y_ld]
    int y_ld;
    float2* y_stats;        // null or [B][tiles per image][N] partial (sum, sumsq) of the stored bf16 values
    float* y_nchw;          // if set: fp32 NCHW output [B][N][Wout][Hout] instead of y
    // split-K over channel chunks
    int ksplit;             // >= 1
    float* slab;            // [tiles][ksplit][BM*BN] fp32 (ksplit > 1)
    int* ticket;            // [tiles] zero-initialised arrival counters (re-armed by the last arriver)
    int lds_total;           // dynamic LDS bytes of the launch (set by launch_conv)
    float gn_inv_n;          // conv_small.hip: 1 / (pixels per image * channels per group)
    const bf16_t* res;       // conv_small.hip: identity residual [B][Wout][Hout][N] added in the epilogue (or null)
    unsigned long long* ts;  // tuning: s_memtime stamps of blocks 0..3, wave 0 ([4][64]) or null
    int dbg;                // tuning ablations (rldm_debug_set_flags): 1 skip stores, 2 skip main loop, 4 skip GN finalize
    SchedFuse sch;          // conv_igemm.hip, y_nchw outputs: the sampler's scheduler step in the epilogue
    int* step_inc;          // conv_igemm.hip: the sampler's device step index, advanced by the step's FIRST launch (conv_in, which does not read it) or null
    int nviews;             // conv_small.hip, image-owning tiles: normalised copies of the output for up to 3 consumers
    NormView nv[3];
    int st_inst;            // conv_stream.hip: which kernel runs (StreamInst below; host side only, no kernel reads it)
    int exp;                // ... round-4 experiment switches (rldm_debug_set_flags2 >> 8; conv_stream_body.h)
    int* cu_lock;           // ... [4096] zero-initialised per-CU locks (exp & 2)
};

struct ConvTile {
    int BM, BN, CK, taps;
};
// row stride (bytes) of one LDS / packed-weight row for a CK
inline int conv_row_bytes(int CK) { return CK * 2 + 16; }
size_t conv_lds_bytes(const ConvTile& t, const ConvParams& p);
bool conv_tile_supported(const ConvTile& t);
int conv_max_halo_slots(const ConvTile& t);
int conv_halo_col_bytes(const ConvTile& t, int TH, int stride);
int conv_tile_threads(const ConvTile& t);
int launch_conv(const ConvTile& t, const ConvParams& p, hipStream_t stream);

// Activation-stationary stride-1 variant for 64-pixel tiles (conv_small.hip): 3x3 over one pre-activated input tensor
// (C1 == 0, no GroupNorm prologue) or 1x1 with the GroupNorm affine folded in; an identity residual is added in the
// epilogue (ConvParams::res).  wpk is the fragment-ordered image
// [N/32][k-groups][9*Cin/16/KG + R/16/KG][64 lanes][8 bf16] (ConvLayer::get_fragpacked), colb from conv_small_col_bytes,
// BN in {32, 64}, KG = conv_small_kgroups(BN).
int conv_small_kgroups(int BN);
int conv_small_col_bytes(int Cin, int TH, int taps);
size_t conv_small_lds_bytes(const ConvParams& p, int taps, int BN);
bool conv_small_supported(const ConvParams& p, int taps, int BN);
int launch_conv_small(const ConvParams& p, int taps, int BN, hipStream_t stream);

// Weight-streaming 3x3 variant (conv_stream.hip), 64-channel chunks.  Same ConvParams (colb = conv_halo_col_bytes of a CK = 64 tile); wpk
// is the fragment-ordered image [N/32][KG][(Cin/64 * 9 + R/64) * 4/KG k-steps][64 lanes][8 bf16] (ConvLayer::get_streampacked), or the
// sub-pixel instances' summed taps (ConvLayer::get_subpixpacked).
// One row of kStreamInst per compiled kernel, chosen by ConvParams::st_inst.  A row is the kernel's template arguments (conv_stream_body.h
// explains them) plus the preconditions that are the instance's own: the pixel tiles it takes, "no nearest x2 folded into the staging",
// "no residual phase".  Everything else -- threads, tile, k-groups, workgroups per CU, the LDS cap -- follows from the template arguments
// through the functions of the row, which are the ones conv_stream_body computes its constants with.
enum StreamInst : int {
    SI_256x128,             // pixels x channels of a workgroup's tile.  8 waves, one workgroup per CU:
    SI_256x64,              //   layers of 64 (192, ...) output channels: 2 k-groups (the VAE decoder's full-resolution level)
    SI_128x64,              //   the 128x8 level, too few 256-pixel tiles to fill the chip: 4 k-groups; 32 x 4 tiles for images of 4 beams
    SI_256x128_SPEC,        //   conv_stream_spec_kernel: 4 matrix waves + 4 staging waves (Flag2.STREAM_SPEC_WAVES)
    SI_64x128,              //   the 128x8 level: 8 x 8 tiles, two 32-pixel fragments per wave, 2 k-groups
    SI_64x128_S2,           //   ... at stride 2 (Downsample2D); 16 x 4 tiles for outputs of 4 beams
    SI_128x128_W4,          // 4 waves, two workgroups per CU:
    SI_128x64_W4,           //   2 k-groups
    SI_SUB_W4,              //   nearest x2 + 3x3 in its sub-pixel form: the tiles are INPUT tiles, four parity workgroups each
    SI_SUB_T4_W4,           //   ... on 32 x 4 tiles (inputs of 4 beams)
    SI_FULLH_W4,            //   tiles as tall as the image (8 x 16 | 16 x 8): the halo rows above / below are never staged
    SI_COUNT
};
// what a conv_stream phase of the persistent launch runs (trunk.hip, TW_SUB of its record); TSF_NONE: the instance is launched only
enum TrunkStreamForm : int { TSF_NONE = -1, TSF_PLAIN = 0, TSF_SUB = 1, TSF_FULLH = 2 };
struct StreamTile {
    int TW, TH;
};
struct StreamInstDesc {
    int WM, WN, NW = 8, MI = 4, STR = 1;
    bool SUB = false, T4 = false, FH = false;
    bool spec = false;                          // conv_stream_spec_kernel instead of conv_stream_kernel<...>
    StreamTile tiles[2] = {};                   // pixel tiles (TW = 0: no second one)
    bool up1 = false, no_res = false;           // ConvParams::up == 1 only / R0 + R1 == 0 only
    int trunk = TSF_NONE;
    constexpr int threads() const { return 64 * NW; }
    constexpr int kgroups() const { return NW / (WM * WN); }
    constexpr int bm() const { return 32 * MI * WM; }
    constexpr int bn() const { return 32 * WN; }
    constexpr int wg_per_cu() const { return NW == 4 ? 2 : 1; }
    constexpr int lds_cap() const { return 160 * 1024 / wg_per_cu(); }      // (co-resident workgroups share the CU's LDS)
    constexpr bool takes(int TW, int TH) const { return (tiles[0].TW == TW && tiles[0].TH == TH) || (tiles[1].TW == TW && tiles[1].TH == TH); }
};
constexpr StreamInstDesc kStreamInst[SI_COUNT] = {
    //                     WM WN NW MI STR  SUB    T4     FH     spec    tiles               up1    no_res trunk
    /* SI_256x128      */ {2, 4, 8, 4, 1, false, false, false, false, {{32, 8}},          false, false, TSF_PLAIN},
    /* SI_256x64       */ {2, 2, 8, 4, 1, false, false, false, false, {{32, 8}}},
    /* SI_128x64       */ {1, 2, 8, 4, 1, false, false, false, false, {{16, 8}, {32, 4}}},
    /* SI_256x128_SPEC */ {2, 4, 8, 4, 1, false, false, false, true,  {{32, 8}}},
    /* SI_64x128       */ {1, 4, 8, 2, 1, false, false, false, false, {{8, 8}}},
    /* SI_64x128_S2    */ {1, 4, 8, 2, 2, false, false, false, false, {{8, 8}, {16, 4}},  true,  true},
    /* SI_128x128_W4   */ {1, 4, 4, 4, 1, false, false, false, false, {{16, 8}},          false, false, TSF_PLAIN},
    /* SI_128x64_W4    */ {1, 2, 4, 4, 1, false, false, false, false, {{16, 8}}},
    /* SI_SUB_W4       */ {1, 4, 4, 4, 1, true,  false, false, false, {{16, 8}},          true,  true,  TSF_SUB},
    /* SI_SUB_T4_W4    */ {1, 4, 4, 4, 1, true,  true,  false, false, {{32, 4}},          true,  true},
    /* SI_FULLH_W4     */ {1, 4, 4, 4, 1, false, false, true,  false, {{8, 16}, {16, 8}}, true,  false, TSF_FULLH},
};
inline const StreamInstDesc& stream_inst(const ConvParams& p) { return kStreamInst[p.st_inst]; }     // (st_inst: a StreamInst)
int conv_stream_bn(const ConvParams& p);
int conv_stream_kgroups(const ConvParams& p);
size_t conv_stream_lds_bytes(const ConvParams& p);
bool conv_stream_supported(const ConvParams& p, int taps);
int launch_conv_stream(const ConvParams& p, hipStream_t stream);

// conv_regw.hip (round 4): 64 -> 64 channel 3x3 / stride 1 convs over 16 x 8 tiles with the weights resident in registers and a persistent
// tile loop per workgroup (the VAE decoder's full-resolution level).  `p` as for conv_stream (16 x 8 tiles); the output statistics are
// ONE partial per workgroup: y_stats is [B][conv_regw_wg_per_image(p)][N].
size_t conv_regw_lds_bytes();
int conv_regw_wg_per_image(const ConvParams& p);
int conv_regw_partials(const ConvParams& p);
bool conv_regw_supported(const ConvParams& p);
int launch_conv_regw(const ConvParams& p, hipStream_t stream);
// conv_regw.hip, conv_c16_kernel (round 4): the network's input layer -- 3x3 / stride 1 over 16 (padded) input channels, 128 | N, 16 x 8 tiles;
// weights [N / 32][9 taps][64 lanes][8 bf16] (ConvLayer::get_c16packed); advances ConvParams::step_inc like the generic kernel
size_t conv_c16_lds_bytes();
bool conv_c16_supported(const ConvParams& p);
int launch_conv_c16(const ConvParams& p, hipStream_t stream);
// conv_regw.hip, conv_o4_kernel (round 4): the UNet's output layer -- GroupNorm + SiLU -> 3x3 over 128 channels -> <= 4 channels, fp32 NCHW +
// ConvParams::sch (the scheduler step); weights stream-packed with 2 k-groups (ConvLayer::get_streampacked(128, 2))
size_t conv_o4_lds_bytes();
bool conv_o4_supported(const ConvParams& p);
int launch_conv_o4(const ConvParams& p, hipStream_t stream);
// conv_regw.hip, conv_ds2_kernel (round 4): 3x3 / stride 2 / pad 1 over 256 channels, no norm, on 32 x 1 output tiles x 32 channels with the 8
// waves as k-groups (the UNet's 64x4 -> 32x2 down-sampler); weights stream-packed with 2 k-groups; one statistics partial per tile
size_t conv_ds2_lds_bytes();
bool conv_ds2_supported(const ConvParams& p);
int launch_conv_ds2(const ConvParams& p, hipStream_t stream);

// Persistent trunk launch (trunk.hip): consecutive conv_small launches whose tile owns a whole image (<= 64 pixels, 32-channel
// tiles) as the phases of ONE launch; the N / 32 workgroups of an image hand their outputs to each other through the L2 of the
// XCD they share.  `kind`: 0 = 3x3 over 256 channels, 1 = 3x3 over 512, 2 = 1x1 over 256 (conv_small instances <1,2,9,2>,
// <1,4,9,2>, <1,2,1,2>).
// The phase record (TrunkPhase: 64 dwords), its host-side encoders and the kernel's decoders: trunk_record.h.
struct TrunkPhase;
struct TrunkParams {
    const TrunkPhase* phases;   // device
    int nphases;
    int B, ranks;               // images; workgroups per image (its cluster): channel tiles x pixel tiles
    int ntile_n, nwn;           // channel tiles per image and 32-channel tiles per workgroup (N / 32 and 1 for image-owning tiles)
    int variant;                // kernel: 0 image-owning conv_small tiles, 1 multi-tile conv_small clusters, 2 conv_stream<256 px, 128 ch>,
                                // 4 conv_stream<128 px, 128 ch> on 4 waves: 32 workgroups per image, two per CU (round 4)
                                // (each set of instances has its own register allocation; 3 and 5 were 128x8-level variants, removed)
    int skew;                   // variant 4: start delay of the second image group, x 1024 cycles
    unsigned* counters;         // device [B][32] zero-initialised: [0] arrivals (monotonic), [1] rank 0's XCC id + 1, [3] launches so far
    int* error;                 // device flag: 1 a bounded wait gave up, 2 a cluster is spread over several XCDs
    const float* temb;          // the plan's time-embedding table (PlanIO), set per launch
    const int* step_ptr;
    int temb_rows_per_step, temb_per_sample, temb_ld;
    unsigned long long* ts;     // ABLATE builds: [phase][16] s_memtime stamps of workgroup 0 (rldm_debug_timestamps buffer) or null
};
int launch_trunk(const TrunkParams& tp, size_t lds, hipStream_t stream);
int trunk_max_resident(int variant, size_t lds);   // workgroups of that kernel per CU by the runtime's occupancy query (< 0: query failed)

// ---------------------------------------------------------------------------------------------------------------
// Per-channel statistics (norm.hip) for tensors that did not come out of a conv epilogue (tests, external inputs):
// deterministic partial (sum, sumsq) per (b, pixel chunk p, channel).
// ---------------------------------------------------------------------------------------------------------------
struct GnStatsParams {
    const bf16_t* x;        // [B][npix][C]
    int C;
    int B, npix;            // pixels per image
    int P;                  // pixel chunks per image (grid.x)
    float2* part;           // [B][P][C] per-channel (sum, sumsq)
};
int launch_gn_stats(const GnStatsParams& p, hipStream_t stream);

// [B][P][C] partials -> [B][2][C]: the per-image double-precision total as float head + tail (see gn_fold_kernel).
struct GnFoldParams {
    const float2* part;     // [B][P][C]
    float2* out;            // [B][2][C]
    int B, P, C;
};
int launch_gn_fold(const GnFoldParams& p, hipStream_t stream);

// y = silu?( GroupNorm( cat[x0, x1] ) ) as one bf16 tensor [B][npix][C0 + C1], from the producers' per-channel partials.
// Used in front of conv_small.hip where every 32/64-channel tile of a conv would otherwise redo the whole activation.
struct GnApplyParams {
    const bf16_t* x0;
    const bf16_t* x1;
    int C0, C1;
    const float2* st0;
    const float2* st1;
    int P0, P1;
    int B, npix;
    int groups;
    const float* gamma;
    const float* beta;
    float eps;
    int silu;
    bf16_t* y;
    float inv_n;            // 1 / (npix * channels per group) (set by launch_gn_apply)
    // two outputs instead of one (ysplit > 0, a multiple of 8): channels [0, ysplit) -> y [B][npix][ysplit], the rest -> y1
    // [B][npix][Cin - ysplit] -- a concatenation wider than a conv kernel takes is convolved half by half (runtime.hip)
    bf16_t* y1;
    int ysplit;
};
int launch_gn_apply(const GnApplyParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// Multi-head self-attention with head_dim 8 (attention.hip).  qkv: [B][L][3C] (q | k | v, q pre-scaled by
// log2(e)/sqrt(8) through the packed weights), out: [B][L][C].
// ---------------------------------------------------------------------------------------------------------------
struct AttnParams {
    const bf16_t* qkv;
    bf16_t* out;
    int B, L, C;
};
int launch_attention(const AttnParams& p, hipStream_t stream);

// Fused GroupNorm -> q/k/v projection -> attention (attention.hip): x is the block input with its statistics partials;
// wfrag = per-head MFMA A fragments [heads][C/16][64 lanes][8 bf16] (rows 0-7 q pre-scaled by log2(e)/sqrt(8), 8-15 k,
// 16-23 v, 24-31 zero), bias [heads][32] fp32.  out: [B][L][C].
struct AttnQkvParams {
    const bf16_t* x;
    const float2* st;
    int P;
    const float* gamma;
    const float* beta;
    float eps;
    int groups;
    float inv_n;
    int magic_cpg;
    const bf16_t* wfrag;
    const float* bias;
    bf16_t* out;
    int B, L, C;
    unsigned long long* ts;     // ABLATE builds: phase stamps of workgroup 0 + [start, end] of every workgroup, launches with L == ts_L
    int ts_L;
    // fused output projection (round 3; null proj_w: off): y = to_out(attention) + bias + res and y's GroupNorm statistics, computed
    // by the SAME launch once all heads of the image have published their rows (a cluster seam like trunk.hip's: the image's
    // workgroups share an XCD).  proj_w: MFMA A fragments [C/32][C/16][64 lanes][8 bf16]; proj_stats: [B][L/64][C] partials.
    const bf16_t* proj_w;
    const float* proj_bias;
    const bf16_t* proj_res;
    bf16_t* proj_y;
    float2* proj_stats;
    unsigned* proj_counter;     // [B][32] arrival counters (monotonic; [3] = launches so far), zeroed at allocation
    int* proj_error;            // the plan's self-check word (1: a wait gave up, 2: an image's workgroups on several XCDs)
};
int launch_attention_qkv(const AttnQkvParams& p, hipStream_t stream);
// the second-generation launch's geometry for (B, L, C): heads per workgroup and waves; non-zero: it declines this shape
int attention_qkv2_geometry(int B, int L, int C, int* HG, int* waves);
// ... and whether that launch can carry the output projection (workgroups of an image = 64-pixel blocks, all co-resident)
bool attention_proj_fusable(int B, int L, int C, int cus);
int launch_attention_proj(const AttnQkvParams& p, hipStream_t stream);    // the same tail as a launch of its own (proj_counter unused)
// what launch_attention_qkv runs for (B, L, C) (tests): route[0] = 2 (attention_qkv2_d8_kernel) or 1 (attention_qkv_d8_kernel), [1] PAIR,
// [2] HG, [3] waves per workgroup, [4] attention_proj_fusable for the shape alone, [5] the same on `cus` compute units
void attention_qkv_route(int B, int L, int C, int cus, int* route);
// LDS of the second-generation fused attention body (attention_body.h) for HG heads per workgroup on `waves` waves: K rows, V^T,
// the GroupNorm affine + scratch, the heads' W' fragments and biases, and one 32-row x 144-byte x staging tile per wave
constexpr int kAttnXRowBytes = 128 + 16, kAttnXStageBytes = 32 * kAttnXRowBytes;
inline size_t attention_qkv2_lds_bytes(int L, int C, int HG, int waves) {
    const size_t Lp = (size_t)(L + 31) / 32 * 32;
    const size_t a = (size_t)2 * C * 8, b2 = (size_t)HG * (C / 16) * 64 * 4;
    return HG * Lp * 16 + (size_t)HG * 10 * (Lp + 8) * 2 + 16 + (size_t)C * 8 + (a > b2 ? a : b2) + (size_t)HG * C * 64 +
           (size_t)HG * 128 + (size_t)waves * kAttnXStageBytes + 128;
}

// ---------------------------------------------------------------------------------------------------------------
// Small kernels (elementwise.hip)
// ---------------------------------------------------------------------------------------------------------------
// conv_in input: [B][W][H][Cpad] bf16 from fp32 NCHW sources: x (cx ch, * scale), pos-encoding channel, cond (cc ch)
struct PackInputParams {
    const float* x; int cx; float scale;
    int pos_encoding;
    const float* cond; int cc;
    int B, W, H, Cpad;
    bf16_t* out;
    int* step_inc;            // sampler: the device step index is advanced here, by the first launch of a step (or null)
};
int launch_pack_input(const PackInputParams& p, hipStream_t stream);
int launch_nchw_f32_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, int W, int H, int Cpad, hipStream_t s);
int launch_nhwc_bf16_to_nchw_f32(const bf16_t* src, float* dst, int B, int C, int W, int H, int ld, hipStream_t s);

// time embedding + all per-resnet projections for `rows` timesteps:
//   e=[cos(t f), sin(t f)] (dim0) -> Linear(dim0, D) -> SiLU -> Linear(D, D) -> SiLU -> Linear(D, total) (+bias)
struct TembParams {
    const float* t;          // [rows] timesteps as float (device)
    int rows, dim0, D, total;
    const float* w1; const float* b1;   // [D][dim0]
    const float* w2; const float* b2;   // [D][D]
    const float* wp; const float* bp;   // [total][D] concatenated time_emb_proj
    float* out;              // [rows][total]
    float* scratch;          // [2][rows][D] (the two hidden layers)
    int flip_sin_to_cos, freq_shift;   // diffusers Timesteps arguments: UNet2DModel (1, 0); sgm get_timestep_embedding (0, 1)
};
int launch_temb(const TembParams& p, hipStream_t stream);

// scheduler steps; coef on host (baked) or read from device table row *step_ptr
struct SchedParams {
    int mode;                 // 0 ddim, 1 ddpm; | prediction type << 1 | kSchedMultistep (sched_prev)
    float coef[5];
    const float* coef_table;  // device [steps][5] or null
    const int* step_ptr;
    const float* eps; const float* x; const float* noise;   // noise may be null; multistep mode: the x0 history (rewritten)
    long long noise_step_stride;                            // elements between steps in `noise` (table mode)
    float* x_prev;
    long long n;
};
int launch_sched_step(const SchedParams& p, hipStream_t stream);
// guided scheduler step: the step of `s`, then the known-region blend and the re-noise (elementwise.hip).  In table mode the rows
// are 9 floats wide ({coef[5], ka, kb, ra, rb}) and the three noise tensors share s.noise_step_stride; s.n = B * per_sample.
struct GuidedSchedParams {
    SchedParams s;
    float k[4];                       // ka, kb, ra, rb (baked mode)
    const float* known;               // z0, laid out like x
    const float* mask;                // [B][spatial], 1 = known
    const float* known_noise;         // nk, like noise; may be null when kb == 0 on every row
    const float* renoise_noise;       // nr, like noise; may be null when no row jumps
    long long per_sample;             // channels * spatial
    long long spatial;
};
int launch_sched_guided_step(const GuidedSchedParams& p, hipStream_t stream);
// UniPC step (elementwise.hip, sched_unipc_kernel): the row {alpha, s, use_corr, k_last, k_1, k_2, k_3, k_t, p_x, p_0, p_1, p_2} of
// rldm_sched_unipc_step, baked or row *step_ptr of a [steps][12] device table.  last [n] and hist [3][n] are the solver's state, read
// (only under a non-zero coefficient) and rewritten element-wise by the same thread; they alias nothing.  x_prev may be x itself.
struct UniPCParams {
    int pred;                 // RLDM_PRED_*
    float coef[12];
    const float* coef_table;  // device [steps][12] or null
    const int* step_ptr;
    const float* out;         // the model output
    const float* x;
    float* last;
    float* hist;
    float* x_prev;
    long long n;
};
int launch_sched_unipc_step(const UniPCParams& p, hipStream_t stream);
int launch_add_noise(const float* x0, const float* noise, const float* sa, const float* sb, int B, long long per,
                     float* out, hipStream_t stream);
int launch_diag_gaussian(const float* moments, const float* noise, float scale, int B, int z, int spatial, float* out,
                         hipStream_t stream);
int launch_step_counter(int* step_ptr, int set_to, int increment, hipStream_t stream);
int launch_trunk_check(const int* err, float* a, long long na, float* b, long long nb, hipStream_t stream);   // NaN-poison on a tripped self-check
int launch_stamp(unsigned long long* slot, hipStream_t stream);   // *slot = wall_clock64() (100 MHz)
int launch_scale_f32(const float* src, float* dst, float scale, long long n, hipStream_t stream);

// rng.hip: out[b][e] = normal(seed, 4 * draw + purpose, row, sample0 + b, e) for b < B, e < per_sample (include/rangeldm_hip.h).
// Immediate form: record == null, the generator is (seed, draw, sample0) and the row is `row`.  Sampler form (inside a captured
// graph): record -> {seed low, seed high, draw, sample offset} on the device, the first sample is record[3] + sample0, and the row
// is *step_ptr + row (step_ptr may be null: row).
struct RngFillParams {
    float* out;
    long long per_sample;
    int B;
    unsigned purpose;
    unsigned long long seed;
    unsigned draw, row, sample0;
    const unsigned* record;
    const int* step_ptr;
};
int launch_rng_fill(const RngFillParams& p, hipStream_t stream);
int launch_rng_record(unsigned* record, unsigned long long seed, unsigned draw, unsigned sample_offset, hipStream_t stream);

}  // namespace rldm
