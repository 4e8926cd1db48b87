// rangenet.hip -- RangeNet++ (DarkNet21 / DarkNet53 backbone, DarkNet decoder, 3x3 head) inference: the network whose last
// decoder feature map is the FRD activation and whose per-pixel argmax is the segmentation.
//
// One implicit-GEMM kernel family, rn_conv_kernel<KIND>, on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
//   KIND 1x1      BasicBlock conv1
//   KIND 3x3      stem, BasicBlock conv2, head          zero padding on BOTH axes (a range image is NOT wrapped here)
//   KIND 3x3 S2   the encoder's down-samplers           stride (1, 2): the azimuth alone is halved
//   KIND UPCONV   ConvTranspose2d [1,4] / [1,2] / [0,1] as two 2-tap convs by output-column parity (blockIdx.x & 1):
//                     out[2j] = W[1] x[j] + W[3] x[j-1]        out[2j+1] = W[2] x[j] + W[0] x[j+1]
// Activations are bf16 channels-last [B][H][W][pitch(C)], pitch(C) = C rounded up to 16 (pad channels hold zeros).  A layer is
//     acc = sum_taps W . X ;  v = acc * scale[c] + shift[c] ;  v = v >= 0 ? v : 0.1f * v ;  v = v + add0 + add1 ;  out = bf16(v)
// in that order, every step one fp32 operation (the file is compiled without FMA contraction, so the host restatement in
// rangenet.py can follow it bit for bit on operands whose sums are exact).
//
// Tile: the MFMA's A operand is a 32-output-channel weight panel (read from the pre-packed, L2-resident weight image, one 16-byte
// load per lane), its B operand 32 consecutive output columns of one row, read from an LDS halo tile staged once per channel chunk.
// A wave owns RN_TH rows x 32 columns x 32 channels; the four waves of a workgroup share the halo tile and split into WN channel
// panels x 4 / WN row groups.  The accumulator has the pixel on the lane and 16 channels in registers, so the epilogue's channel
// argmax is 15 compares and one cross-half exchange.
#include "common.h"
#include "../../include/rangeldm_hip.h"

#include <cstring>
#include <vector>

namespace {

using namespace rldm;

constexpr int RN_THREADS = 256;
constexpr int RN_TH = 4;             // output rows per wave
constexpr int RN_TILE_W = 32;        // output columns per workgroup (one MFMA N)
constexpr int RN_LDS_MAX = 160 * 1024;   // (the network's own layers stay below 64 KiB; a stride-2 conv into 32 channels needs 94)

inline int rn_pitch(int c) { return (c + 15) & ~15; }
inline int rn_taps(int kind) { return kind == RLDM_RN_CONV1X1 ? 1 : kind == RLDM_RN_UPCONV ? 4 : 9; }
inline bool rn_kind_ok(int kind) { return kind >= RLDM_RN_CONV1X1 && kind <= RLDM_RN_UPCONV; }
inline int rn_out_w(int kind, int W) { return kind == RLDM_RN_CONV3X3_S2 ? (W - 1) / 2 + 1 : kind == RLDM_RN_UPCONV ? 2 * W : W; }

struct RnArgs {
    const bf16_t* x;
    const bf16_t* w;
    const float* scale;
    const float* shift;
    const bf16_t* add0;
    const bf16_t* add1;
    bf16_t* out;
    float* out_f32;
    const uint32_t* gmask;
    const int32_t* gslot;
    float* gathered;
    uint8_t* argmax;
    int H, W, Wout, Cin_p, Cout, Cout_p, nK16, ntiles, KC, WN, R, cogroups, leaky, n_gather;
};

template <int KIND>
__global__ __launch_bounds__(RN_THREADS) void rn_conv_kernel(const RnArgs a) {
    constexpr int S = KIND == RLDM_RN_CONV3X3_S2 ? 2 : 1;
    constexpr int PADY = (KIND == RLDM_RN_CONV3X3 || KIND == RLDM_RN_CONV3X3_S2) ? 1 : 0;
    constexpr int PADX = KIND == RLDM_RN_CONV1X1 ? 0 : 1;
    constexpr int T = KIND == RLDM_RN_CONV1X1 ? 1 : KIND == RLDM_RN_UPCONV ? 4 : 9;      // taps in the packed image
    constexpr int NT = KIND == RLDM_RN_UPCONV ? 2 : T;                                   // taps of one output
    constexpr int COLS_IN = (RN_TILE_W - 1) * S + 1 + 2 * PADX;
    extern __shared__ __align__(16) bf16_t lds[];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    int bx = blockIdx.x, par = 0;
    if (KIND == RLDM_RN_UPCONV) { par = bx & 1; bx >>= 1; }
    const int j0 = bx * RN_TILE_W;
    const int row0 = blockIdx.y * a.R;
    const int b = blockIdx.z / a.cogroups, cog = blockIdx.z % a.cogroups;
    const int cot = cog * a.WN + wave % a.WN, rg = wave / a.WN;
    const bool active = cot < a.ntiles;
    const int rows_in = a.R + 2 * PADY;
    const int KC = a.KC, PITCH = KC + 8, upp = KC >> 3;

    f32x16 acc[RN_TH];
#pragma unroll
    for (int t = 0; t < RN_TH; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    for (int c0 = 0; c0 < a.Cin_p; c0 += KC) {
        __syncthreads();                                 // the previous chunk's reads are done
        const int nunits = rows_in * COLS_IN * upp;
        for (int u = tid; u < nunits; u += RN_THREADS) {
            const int k8 = u % upp, px = u / upp;
            const int lx = px % COLS_IN, ly = px / COLS_IN;
            const int iy = row0 + ly - PADY, ix = j0 * S + lx - PADX;
            uint4 v = {0u, 0u, 0u, 0u};                  // zeros outside the image, on both axes
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = *reinterpret_cast<const uint4*>(a.x + ((size_t)(b * a.H + iy) * a.W + ix) * a.Cin_p + c0 + k8 * 8);
            *reinterpret_cast<uint4*>(lds + px * PITCH + k8 * 8) = v;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                int dy, dx, wt;
                if (KIND == RLDM_RN_UPCONV) { dy = 0; dx = t == 0 ? 0 : (par ? 1 : -1); wt = t == 0 ? (par ? 2 : 1) : (par ? 0 : 3); }
                else if (KIND == RLDM_RN_CONV1X1) { dy = 0; dx = 0; wt = 0; }
                else { dy = t / 3 - 1; dx = t % 3 - 1; wt = t; }
                const int lx = r * S + dx + PADX;
                for (int kk = 0; kk < (KC >> 4); ++kk) {
                    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(
                        a.w + ((size_t)(cot * a.nK16 + (c0 >> 4) + kk) * T + wt) * 512 + lane * 8);
#pragma unroll
                    for (int tt = 0; tt < RN_TH; ++tt) {
                        const int ly = rg * RN_TH + tt + dy + PADY;
                        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(lds + (ly * COLS_IN + lx) * PITCH + kk * 16 + 8 * h);
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[tt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!active) return;                                 // (no barrier follows)

    // epilogue: lane (r, h) holds column j0 + r, channels cot * 32 + 8 g + 4 h + i in register 4 g + i
    const int j = j0 + r;
    const int ox = KIND == RLDM_RN_UPCONV ? 2 * j + par : j;
    const int jmax = KIND == RLDM_RN_UPCONV ? a.W : a.Wout;
    float sc[16], sh[16];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cot * 32 + 8 * g + 4 * h + i;
            sc[4 * g + i] = c < a.Cout ? a.scale[c] : 0.0f;
            sh[4 * g + i] = c < a.Cout ? a.shift[c] : 0.0f;
        }
#pragma unroll
    for (int tt = 0; tt < RN_TH; ++tt) {
        const int oy = row0 + rg * RN_TH + tt;
        const bool inside = oy < a.H && j < jmax;        // (the exchange below runs on every lane)
        const size_t pix = inside ? (size_t)(b * a.H + oy) * a.Wout + ox : 0;
        float best = 0.0f;
        int best_c = -1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = cot * 32 + 8 * g + 4 * h;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t = acc[tt][4 * g + i] * sc[4 * g + i];
                t = t + sh[4 * g + i];
                if (a.leaky) t = t >= 0.0f ? t : 0.1f * t;
                v[i] = t;
            }
            if (inside && cb < a.Cout_p) {
                if (a.add0) {
                    const uint2 q = *reinterpret_cast<const uint2*>(a.add0 + pix * a.Cout_p + cb);
                    v[0] = v[0] + bf16lo(q.x); v[1] = v[1] + bf16hi(q.x); v[2] = v[2] + bf16lo(q.y); v[3] = v[3] + bf16hi(q.y);
                }
                if (a.add1) {
                    const uint2 q = *reinterpret_cast<const uint2*>(a.add1 + pix * a.Cout_p + cb);
                    v[0] = v[0] + bf16lo(q.x); v[1] = v[1] + bf16hi(q.x); v[2] = v[2] + bf16lo(q.y); v[3] = v[3] + bf16hi(q.y);
                }
                if (a.out) {
                    uint2 q;
                    q.x = pack_bf16x2(v[0], v[1]);
                    q.y = pack_bf16x2(v[2], v[3]);
                    *reinterpret_cast<uint2*>(a.out + pix * a.Cout_p + cb) = q;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = cb + i;
                    if (c >= a.Cout) continue;
                    const size_t flat = ((size_t)c * a.H + oy) * a.Wout + ox;        // index into one image's (C, H, W)
                    if (a.out_f32) a.out_f32[(size_t)b * a.Cout * a.H * a.Wout + flat] = v[i];
                    if (a.gathered && ((a.gmask[flat >> 5] >> (flat & 31)) & 1u))
                        a.gathered[(size_t)b * a.n_gather + a.gslot[flat]] = v[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (cb + i < a.Cout && (best_c < 0 || v[i] > best)) { best = v[i]; best_c = cb + i; }     // ascending c: lowest index on ties
        }
        if (a.argmax) {                                  // Cout <= 32: one panel, the other 16 channels are on lane ^ 32
            const float ov = __shfl_xor(best, 32);
            const int oc = __shfl_xor(best_c, 32);
            if (oc >= 0 && (best_c < 0 || ov > best || (ov == best && oc < best_c))) { best = ov; best_c = oc; }
            if (inside && h == 0) a.argmax[pix] = (uint8_t)best_c;
        }
    }
}

// proj fp32 (B, C, H, W) -> bf16 [B][H][W][pitch(C)], pad channels zero
__global__ __launch_bounds__(RN_THREADS) void rn_pack_input_kernel(const float* __restrict__ proj, int C, int Cp, size_t hw, size_t total,
                                                                  bf16_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RN_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % Cp);
    const size_t p = i / Cp, b = p / hw, s = p % hw;
    out[i] = c < C ? f32_to_bf16(proj[(b * C + c) * hw + s]) : (bf16_t)0;
}

int rn_launch(const rldm_rangenet_layer_desc* d, const void* x, const void* w, const float* scale, const float* shift, const void* add0,
              const void* add1, void* out, float* out_f32, const uint32_t* gmask, const int32_t* gslot, int n_gather, float* gathered,
              uint8_t* argmax, hipStream_t stream) {
    RLDM_REQUIRE(d && x && w && scale && shift, "rldm_rangenet_layer: null argument");
    RLDM_REQUIRE(rn_kind_ok(d->kind), "rldm_rangenet_layer: unknown kind");
    RLDM_REQUIRE(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->Cin >= 1 && d->Cout >= 1, "rldm_rangenet_layer: empty shape");
    RLDM_REQUIRE(out || out_f32 || gathered || argmax, "rldm_rangenet_layer: no output requested");
    RLDM_REQUIRE(!argmax || d->Cout <= 32, "rldm_rangenet_layer: the argmax epilogue takes at most 32 channels");
    RLDM_REQUIRE(!gathered || (gmask && gslot && n_gather >= 1), "rldm_rangenet_layer: a gather needs its mask and slot map");
    RnArgs a;
    a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.scale = scale; a.shift = shift;
    a.add0 = (const bf16_t*)add0; a.add1 = (const bf16_t*)add1; a.out = (bf16_t*)out; a.out_f32 = out_f32;
    a.gmask = gmask; a.gslot = gslot; a.gathered = gathered; a.argmax = argmax;
    a.H = d->H; a.W = d->W; a.Wout = rn_out_w(d->kind, d->W);
    a.Cin_p = rn_pitch(d->Cin); a.Cout = d->Cout; a.Cout_p = rn_pitch(d->Cout);
    a.nK16 = a.Cin_p / 16; a.ntiles = (d->Cout + 31) / 32;
    a.KC = a.Cin_p % 32 == 0 ? 32 : 16;
    a.WN = a.ntiles >= 4 ? 4 : a.ntiles >= 2 ? 2 : 1;
    a.R = RN_TH * (4 / a.WN);
    a.cogroups = (a.ntiles + a.WN - 1) / a.WN;
    a.leaky = d->leaky; a.n_gather = n_gather;
    const long long px_in = (long long)d->B * d->H * d->W, px_out = (long long)d->B * d->H * a.Wout;
    RLDM_REQUIRE(px_in * a.Cin_p < (1ll << 31) && px_out * (a.Cout_p > a.Cout ? a.Cout_p : a.Cout) < (1ll << 31),
                 "rldm_rangenet_layer: a tensor of 2^31 elements or more");
    const int pady = (d->kind == RLDM_RN_CONV3X3 || d->kind == RLDM_RN_CONV3X3_S2) ? 1 : 0;
    const int padx = d->kind == RLDM_RN_CONV1X1 ? 0 : 1;
    const int cols_in = (RN_TILE_W - 1) * (d->kind == RLDM_RN_CONV3X3_S2 ? 2 : 1) + 1 + 2 * padx;
    const size_t lds = (size_t)(a.R + 2 * pady) * cols_in * (a.KC + 8) * sizeof(bf16_t);
    RLDM_REQUIRE(lds <= (size_t)RN_LDS_MAX, "rldm_rangenet_layer: halo tile above the LDS of a CU");
    const int nj = d->kind == RLDM_RN_UPCONV ? d->W : a.Wout;
    const long long gx = (long long)((nj + RN_TILE_W - 1) / RN_TILE_W) * (d->kind == RLDM_RN_UPCONV ? 2 : 1);
    const long long gy = (d->H + a.R - 1) / a.R, gz = (long long)d->B * a.cogroups;
    RLDM_REQUIRE(gx < (1ll << 31) && gy <= 65535 && gz <= 65535, "rldm_rangenet_layer: grid too large");
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
#define RN_LAUNCH(KIND)                                                                                          \
    do {                                                                                                         \
        static DynLdsLimit limit;                                                                                \
        RLDM_HIP_CHECK(limit.ensure(reinterpret_cast<const void*>(&rn_conv_kernel<KIND>), lds));                \
        hipLaunchKernelGGL(rn_conv_kernel<KIND>, grid, dim3(RN_THREADS), lds, stream, a);                        \
    } while (0)
    switch (d->kind) {
        case RLDM_RN_CONV1X1: RN_LAUNCH(RLDM_RN_CONV1X1); break;
        case RLDM_RN_CONV3X3: RN_LAUNCH(RLDM_RN_CONV3X3); break;
        case RLDM_RN_CONV3X3_S2: RN_LAUNCH(RLDM_RN_CONV3X3_S2); break;
        default: RN_LAUNCH(RLDM_RN_UPCONV); break;
    }
#undef RN_LAUNCH
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

struct RnLayer {
    rldm_rangenet_layer_desc d;      // B / H / W are filled in per forward
    bf16_t* w = nullptr;             // device, packed
    float* scale = nullptr;          // device [Cout]
    float* shift = nullptr;
};

}  // namespace

struct rldm_rangenet {
    rldm_rangenet_config cfg;
    std::vector<RnLayer> layers;
    char* arena = nullptr;
    size_t arena_bytes = 0;
    ~rldm_rangenet() {
        for (auto& l : layers) {
            if (l.w) (void)hipFree(l.w);
            if (l.scale) (void)hipFree(l.scale);
            if (l.shift) (void)hipFree(l.shift);
        }
        if (arena) (void)hipFree(arena);
    }
};

namespace {

const int RN_BLOCKS21[5] = {1, 1, 2, 2, 1};
const int RN_BLOCKS53[5] = {1, 2, 8, 8, 4};
const int* rn_blocks(int layers) { return layers == 21 ? RN_BLOCKS21 : layers == 53 ? RN_BLOCKS53 : nullptr; }

// (kind, Cin, Cout, leaky) of every layer in walk order: stem; enc1..5 (down, then conv1 / conv2 per block); dec5..1 (upconv, conv1,
// conv2); head
std::vector<rldm_rangenet_layer_desc> rn_layer_list(const rldm_rangenet_config& cfg) {
    std::vector<rldm_rangenet_layer_desc> v;
    auto push = [&](int kind, int cin, int cout, int leaky) { v.push_back({kind, 0, 0, 0, cin, cout, leaky}); };
    const int* blocks = rn_blocks(cfg.layers);
    push(RLDM_RN_CONV3X3, cfg.in_channels, 32, 1);
    int c = 32;
    for (int l = 0; l < 5; ++l) {
        push(RLDM_RN_CONV3X3_S2, c, 2 * c, 1);
        for (int k = 0; k < blocks[l]; ++k) {
            push(RLDM_RN_CONV1X1, 2 * c, c, 1);
            push(RLDM_RN_CONV3X3, c, 2 * c, 1);
        }
        c *= 2;
    }
    for (int l = 0; l < 5; ++l) {
        push(RLDM_RN_UPCONV, c, c / 2, 1);
        push(RLDM_RN_CONV1X1, c / 2, c, 1);
        push(RLDM_RN_CONV3X3, c, c / 2, 1);
        c /= 2;
    }
    push(RLDM_RN_CONV3X3, 32, cfg.num_classes, 0);
    return v;
}

}  // namespace

extern "C" {

long long rldm_rangenet_packed_elems(int kind, int Cin, int Cout) {
    if (!rn_kind_ok(kind) || Cin < 1 || Cout < 1) return -1;
    return (long long)((Cout + 31) / 32) * (rn_pitch(Cin) / 16) * rn_taps(kind) * 512;
}

int rldm_rangenet_pack_weights(int kind, int Cin, int Cout, const float* w, uint16_t* packed) {
    RLDM_REQUIRE(rn_kind_ok(kind) && Cin >= 1 && Cout >= 1 && w && packed, "rldm_rangenet_pack_weights: bad argument");
    const int T = rn_taps(kind), nK16 = rn_pitch(Cin) / 16, ntiles = (Cout + 31) / 32;
    for (int cot = 0; cot < ntiles; ++cot)
        for (int k16 = 0; k16 < nK16; ++k16)
            for (int t = 0; t < T; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int jj = 0; jj < 8; ++jj) {
                        const int co = cot * 32 + (lane & 31), k = k16 * 16 + 8 * (lane >> 5) + jj;
                        const float v = (co < Cout && k < Cin) ? w[((size_t)co * T + t) * Cin + k] : 0.0f;
                        packed[(((size_t)(cot * nK16 + k16) * T + t) * 64 + lane) * 8 + jj] = f32_to_bf16(v);
                    }
    return 0;
}

int rldm_rangenet_layer(const rldm_rangenet_layer_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                        const void* add0, const void* add1, void* out, float* out_f32, const uint32_t* gather_mask,
                        const int32_t* gather_slot, int n_gather, float* gathered, uint8_t* argmax, void* stream) {
    return rn_launch(d, x, w_packed, scale, shift, add0, add1, out, out_f32, gather_mask, gather_slot, n_gather, gathered, argmax,
                     (hipStream_t)stream);
}

int rldm_rangenet_num_layers(const rldm_rangenet_config* cfg) {
    if (!cfg || !rn_blocks(cfg->layers)) return -1;
    return (int)rn_layer_list(*cfg).size();
}

int rldm_rangenet_layer_info(const rldm_rangenet_config* cfg, int index, rldm_rangenet_layer_desc* out) {
    RLDM_REQUIRE(cfg && out && rn_blocks(cfg->layers), "rldm_rangenet_layer_info: DarkNet21 or DarkNet53 only");
    const auto list = rn_layer_list(*cfg);
    RLDM_REQUIRE(index >= 0 && index < (int)list.size(), "rldm_rangenet_layer_info: no such layer");
    *out = list[index];
    return 0;
}

int rldm_rangenet_create(const rldm_rangenet_config* cfg, const float* const* weights, const float* const* scale,
                         const float* const* shift, int n_layers, rldm_rangenet** out) {
    RLDM_REQUIRE(cfg && weights && scale && shift && out, "rldm_rangenet_create: null argument");
    RLDM_REQUIRE(rn_blocks(cfg->layers), "rldm_rangenet_create: DarkNet21 or DarkNet53 only");
    RLDM_REQUIRE(cfg->in_channels >= 1 && cfg->in_channels <= 16, "rldm_rangenet_create: 1..16 input channels");
    RLDM_REQUIRE(cfg->num_classes >= 1 && cfg->num_classes <= 32, "rldm_rangenet_create: 1..32 classes");
    const auto list = rn_layer_list(*cfg);
    RLDM_REQUIRE(n_layers == (int)list.size(), "rldm_rangenet_create: layer count does not match the architecture");
    auto* net = new rldm_rangenet();
    net->cfg = *cfg;
    net->layers.resize(list.size());
    std::vector<uint16_t> packed;
    int rc = 0;
    for (size_t i = 0; i < list.size() && !rc; ++i) {
        RnLayer& l = net->layers[i];
        l.d = list[i];
        if (!weights[i] || !scale[i] || !shift[i]) { rldm::set_error("rldm_rangenet_create: layer " + std::to_string(i) + " has no weights"); rc = 1; break; }
        packed.resize((size_t)rldm_rangenet_packed_elems(l.d.kind, l.d.Cin, l.d.Cout));
        rc = rldm_rangenet_pack_weights(l.d.kind, l.d.Cin, l.d.Cout, weights[i], packed.data());
        auto up = [&](void** dst, const void* src, size_t bytes) {
            if (hipMalloc(dst, bytes) != hipSuccess || hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
                rldm::set_error("rldm_rangenet_create: device allocation or upload of layer " + std::to_string(i) + " failed");
                return 1;
            }
            return 0;
        };
        rc = rc || up((void**)&l.w, packed.data(), packed.size() * sizeof(uint16_t)) ||
             up((void**)&l.scale, scale[i], (size_t)l.d.Cout * sizeof(float)) || up((void**)&l.shift, shift[i], (size_t)l.d.Cout * sizeof(float));
    }
    if (rc) { delete net; return 1; }
    *out = net;
    return 0;
}

void rldm_rangenet_destroy(rldm_rangenet* net) { delete net; }

int rldm_rangenet_forward(rldm_rangenet* net, const float* proj, int B, int H, int W, const uint32_t* gather_mask,
                          const int32_t* gather_slot, int n_gather, float* features, uint8_t* argmax, float* logits, void* stream_) {
    RLDM_REQUIRE(net && proj, "rldm_rangenet_forward: null argument");
    RLDM_REQUIRE(B >= 1 && H >= 1 && W >= 32 && W % 32 == 0, "rldm_rangenet_forward: the width must be a multiple of 32 (five halvings)");
    RLDM_REQUIRE(n_gather == 0 || (gather_mask && gather_slot && features), "rldm_rangenet_forward: a gather needs mask, slots and output");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t unit = (size_t)B * H * W * 32 * sizeof(bf16_t);    // a C-channel map at width W * 32 / C: the same bytes at every level
    // arena: input | stem | keep[5] | scratch | mid (unit / 2) | d | dm (2 units) | e[2]
    const size_t need = unit * 14;
    if (net->arena_bytes < need) {
        RLDM_HIP_CHECK(hipStreamSynchronize(stream));
        if (net->arena) RLDM_HIP_CHECK(hipFree(net->arena));
        net->arena = nullptr;
        net->arena_bytes = 0;
        RLDM_HIP_CHECK(hipMalloc((void**)&net->arena, need));
        net->arena_bytes = need;
    }
    auto buf = [&](int i) { return (void*)(net->arena + unit * i); };
    void* in = buf(0);
    void* stem = buf(1);
    void* keep[5] = {buf(2), buf(3), buf(4), buf(5), buf(6)};
    void* scratch = buf(7);
    void* mid = buf(8);
    void* dbuf = buf(9);
    void* dm = buf(10);              // two units
    void* e[2] = {buf(12), buf(13)};

    const int Cp = rn_pitch(net->cfg.in_channels);
    RLDM_REQUIRE((size_t)B * H * W * Cp * sizeof(bf16_t) <= unit, "rldm_rangenet_forward: input pitch above 32 channels");
    {
        const size_t total = (size_t)B * H * W * Cp;
        hipLaunchKernelGGL(rn_pack_input_kernel, dim3((unsigned)((total + RN_THREADS - 1) / RN_THREADS)), dim3(RN_THREADS), 0, stream, proj,
                           net->cfg.in_channels, Cp, (size_t)H * W, total, (bf16_t*)in);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    size_t li = 0;
    auto run = [&](int w_in, const void* x, const void* a0, const void* a1, void* o, float* of32, bool gather, uint8_t* am) {
        RnLayer& l = net->layers[li++];
        l.d.B = B; l.d.H = H; l.d.W = w_in;
        return rn_launch(&l.d, x, l.w, l.scale, l.shift, a0, a1, o, of32, gather ? gather_mask : nullptr, gather ? gather_slot : nullptr,
                         gather ? n_gather : 0, gather ? features : nullptr, am, stream);
    };
    const int* blocks = rn_blocks(net->cfg.layers);
    if (run(W, in, nullptr, nullptr, stem, nullptr, false, nullptr)) return 1;
    const void* skips[5];
    const void* cur = stem;
    int w = W;
    for (int l = 0; l < 5; ++l) {
        skips[l] = cur;                                  // the INPUT of the down-sampler, at os = 2^l
        // the blocks ping-pong between keep[l] and scratch; start so that the last one lands in keep[l]
        void* a = blocks[l] % 2 ? scratch : keep[l];
        void* bb = blocks[l] % 2 ? keep[l] : scratch;
        if (run(w, cur, nullptr, nullptr, a, nullptr, false, nullptr)) return 1;
        w /= 2;
        for (int k = 0; k < blocks[l]; ++k) {
            if (run(w, a, nullptr, nullptr, mid, nullptr, false, nullptr)) return 1;
            if (run(w, mid, a, nullptr, bb, nullptr, false, nullptr)) return 1;
            void* t = a; a = bb; bb = t;
        }
        cur = a;                                         // == keep[l]
    }
    for (int l = 4; l >= 0; --l) {
        if (run(w, cur, nullptr, nullptr, dbuf, nullptr, false, nullptr)) return 1;
        w *= 2;
        if (run(w, dbuf, nullptr, nullptr, dm, nullptr, false, nullptr)) return 1;
        const bool last = l == 0;
        float* f32 = last && n_gather == 0 ? features : nullptr;
        if (run(w, dm, dbuf, skips[l], e[l & 1], f32, last && n_gather > 0, nullptr)) return 1;
        cur = e[l & 1];
    }
    RLDM_REQUIRE(argmax || logits, "rldm_rangenet_forward: neither argmax nor logits requested");
    if (run(w, cur, nullptr, nullptr, nullptr, logits, false, argmax)) return 1;
    return 0;
}

}  // extern "C"
