// Internal header of the inference runtime: what weights.hip (parameter store, weight packers), plan.hip (plan builder, routing
// state), runtime.hip (networks, their walks and C entry points), sampler.hip and test_entry.hip share.  Host code only.
#pragma once
#include "../../include/rangeldm_hip.h"
#include "kernels.h"
#include "trunk_seam.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

namespace rldm {

// ---------------------------------------------------------------------------------------------------------------
// device memory helpers
// ---------------------------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int alloc(size_t n) {
        reset();
        if (n == 0) n = 16;
        RLDM_HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
        return 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

inline int upload(DevBuf& b, const void* host, size_t bytes) {
    if (b.alloc(bytes)) return 1;
    RLDM_HIP_CHECK(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// first-fit offset allocator over one arena; plans are built twice (dry run for the peak, then for real)
struct Arena {
    struct Blk { size_t off, size; };
    std::vector<Blk> free_list;
    size_t top = 0, peak = 0;
    size_t alloc(size_t n) {
        n = (n + 255) & ~(size_t)255;
        for (size_t i = 0; i < free_list.size(); ++i) {
            if (free_list[i].size >= n) {
                size_t off = free_list[i].off;
                free_list[i].off += n;
                free_list[i].size -= n;
                if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
                return off;
            }
        }
        size_t off = top;
        top += n;
        peak = std::max(peak, top);
        return off;
    }
    void release(size_t off, size_t n) {
        n = (n + 255) & ~(size_t)255;
        free_list.push_back({off, n});
        std::sort(free_list.begin(), free_list.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < free_list.size();) {
            if (free_list[i].off + free_list[i].size == free_list[i + 1].off) {
                free_list[i].size += free_list[i + 1].size;
                free_list.erase(free_list.begin() + i + 1);
            } else {
                ++i;
            }
        }
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
            top = free_list.back().off;
            free_list.pop_back();
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// layers: host fp32 parameters + lazily packed device images
// ---------------------------------------------------------------------------------------------------------------
struct NormParams {
    DevBuf gamma, beta;
    int C = 0;
};

struct ConvLayer {
    std::string name;
    int Cout = 0, Cin = 0, ksize = 3;          // real sizes
    std::vector<float> w, b;                   // host fp32, (Cout, Cin, k, k) / (Cout)
    // residual phase fused into this conv's K loop (conv_igemm.hip): a 1x1 map over R channels of the block input.
    // sc_w = conv_shortcut weights (Cout, R) [its bias is folded into b], or empty + sc_identity for a plain `x + h`.
    int R = 0;
    bool sc_identity = false;
    std::vector<float> sc_w;
    struct Packed {
        DevBuf w, bias;
        int Cin_pad = 0;
    };
    // the order a kernel family reads its weights in, and the integers that layout is parameterised by:
    // Igemm (BN, CK), Stream (k-groups), Frag / FragNoRes (channels per tile, k-groups)
    enum class WeightLayout { Igemm, Stream, C16, SubPixel, Frag, FragNoRes };
    using WeightKey = std::tuple<WeightLayout, int, int>;
    std::map<WeightKey, std::unique_ptr<Packed>> packed;

    float weight(int n, int c, int tap) const { return w[((size_t)n * Cin + c) * (ksize * ksize) + tap]; }
    // residual phase: row n of the 1x1 shortcut over the block input, or of the identity
    float res_weight(int n, int c) const { return sc_identity ? (c == n ? 1.f : 0.f) : sc_w[(size_t)n * R + c]; }

    // the image under `key`: built on first use by fill(img, bias) (bias arrives as the layer's own, unpadded), uploaded and kept
    template <class Fill> int cached(const WeightKey& key, int Cin_pad, Packed** out, Fill&& fill) {
        auto it = packed.find(key);
        if (it != packed.end()) {
            RLDM_REQUIRE(it->second->Cin_pad == Cin_pad, "conv layer reused with a different channel padding");
            *out = it->second.get();
            return 0;
        }
        std::vector<bf16_t> img;
        std::vector<float> bias = b;
        if (fill(img, bias)) return 1;
        auto pk = std::make_unique<Packed>();
        if (upload(pk->w, img.data(), img.size() * sizeof(bf16_t))) return 1;
        if (upload(pk->bias, bias.data(), bias.size() * sizeof(float))) return 1;
        pk->Cin_pad = Cin_pad;
        *out = pk.get();
        packed[key] = std::move(pk);
        return 0;
    }

    // the packed images, built on first use (weights.hip states each layout)
    int get_packed(int BN, int CK, int Cin_pad, Packed** out);                     // conv_igemm.hip
    int get_streampacked(int Cin_pad, int KG, Packed** out);                       // conv_stream.hip, conv_regw.hip
    int get_c16packed(Packed** out);                                               // conv_regw.hip, conv_c16_kernel
    int get_subpixpacked(int Cin_pad, Packed** out);                               // conv_stream.hip, sub-pixel form
    int get_fragpacked(int Cin_pad, int TN, int KG, bool no_res, Packed** out);    // conv_small.hip, attention's to_out tail
};

struct ParamStore {
    std::map<std::string, std::vector<float>> host;
    std::map<std::string, int64_t> expected;    // name -> numel
    bool finalized = false;

    int set(const char* name, const float* data, int64_t numel);
    int check_complete() const;
    void expect_conv(const std::string& n, int co, int ci, int k);
    void expect_lin(const std::string& n, int co, int ci);
    void expect_norm(const std::string& n, int c);
    void expect_resnet(const std::string& p, int ci, int co, int temb);
    void expect_attn(const std::string& p, int c);
};

// ---------------------------------------------------------------------------------------------------------------
// execution plan
// ---------------------------------------------------------------------------------------------------------------
struct Tensor {
    size_t off = 0;
    int B = 0, W = 0, H = 0, C = 0;
    int id = -1;
    size_t st_off = 0;     // per-channel partial statistics [B][P][C] float2 (P == 0: none)
    int P = 0;
    int prod = -1;         // ordinal of the Builder::conv call that produced it (-1: something else)
    size_t st_bytes() const { return (size_t)B * P * C * sizeof(float2); }
    size_t bytes() const { return (size_t)B * W * H * C * sizeof(bf16_t); }
    bool valid() const { return id >= 0; }
};

struct PlanIO {
    // conv_in sources (fp32 NCHW, device)
    const float* sample = nullptr;
    int sample_channels = 0;
    float sample_scale = 1.f;
    int pos_encoding = 0;
    const float* cond = nullptr;
    int cond_channels = 0;
    // output (fp32 NCHW, device)
    float* out = nullptr;
    // time-embedding table
    const float* temb = nullptr;
    const int* step_ptr = nullptr;
    int temb_rows_per_step = 1;
    int temb_per_sample = 0;
    // sampler only: the step index advanced by the step's first launch, the scheduler step in conv_out's epilogue
    int* step_inc = nullptr;
    SchedFuse sch = {};
    // sampler only: conv_out's epilogue also writes the next step's conv_in input (sch.pack = xin), so the plan's pack_input launch is
    // skipped and conv_in advances the step index; the sampler packs x_T itself once per call
    bool pack_fused = false;
    bf16_t* xin = nullptr;         // the plan's conv_in input tensor [B][W][H][xin_ld] (never recycled inside the plan)
    int xin_ld = 0;
};

struct Op {
    std::function<int(hipStream_t)> fn;
    std::string name;       // kernel (template instance) the op launches
    double flops = 0;       // algorithmic FLOPs (2*MACs) of this launch
    double bytes = 0;       // algorithmic HBM bytes: every input / weight / output touched once
    std::function<bool()> active;   // optional: false -> the op launches nothing this run (the sampler's fused pack_input) and is skipped
    std::string tag;                // layer name(s), for RLDM_PRINT_PLAN
};

struct KernelStat {
    int launches = 0;
    double ms = 0, flops = 0, bytes = 0;
};

struct Plan {
    int B = 0, W = 0, H = 0;
    int flags = 0;                 // routing options of THIS plan (the bits of rldm_debug_set_flags), in force while it is built
    DevBuf arena;
    DevBuf tickets;                // split-K arrival counters of every conv in the plan
    std::vector<std::unique_ptr<DevBuf>> trunk_bufs;   // phase records / cluster counters of the persistent trunk launches
    DevBuf trunk_error;            // device int: a trunk launch gave up a wait (1) or found a cluster off its XCD (2)
    PlanIO io;
    std::vector<Op> ops;
    double flops = 0;
    int run(hipStream_t s);
    int run_stamped(hipStream_t s, unsigned long long* slots, int cap);            // a timestamp launch around every op
    int run_profiled(hipStream_t s, std::map<std::string, KernelStat>& stats);     // a HIP event pair around every launch
};

struct Layers {
    std::map<std::string, std::unique_ptr<ConvLayer>> conv;
    std::map<std::string, std::unique_ptr<NormParams>> norm;
    ConvLayer* get_conv(const std::string& n) {
        auto it = conv.find(n);
        return it == conv.end() ? nullptr : it->second.get();
    }
    NormParams* get_norm(const std::string& n) {
        auto it = norm.find(n);
        return it == norm.end() ? nullptr : it->second.get();
    }
    int add_conv(ParamStore& ps, const std::string& n, int co, int ci, int k);
    int add_norm(ParamStore& ps, const std::string& n, int c);
    int add_qkv(ParamStore& ps, const std::string& p, int c, int head_dim);
};

// what q is scaled by so that attention works in exp2 units: log2(e) / sqrt(head_dim)
inline float attn_q_scale(int head_dim) { return 1.4426950408889634f / std::sqrt((float)head_dim); }
void pack_attn_head_frags(const float* w, const float* b, int C, std::vector<bf16_t>& img, std::vector<float>& bias);
inline int pad16(int c) { return (c + 15) / 16 * 16; }

struct ConvArgs {
    ConvLayer* layer = nullptr;
    Tensor x0, x1;                 // x1 optional concat
    int stride = 1, pad_mode = 0, up = 1;
    NormParams* gn = nullptr;      // GroupNorm prologue over cat[x0, x1] (needs their statistics)
    float eps = 1e-5f;
    int groups = 32;
    int silu = 0;
    int temb_off = -1;             // channel offset into the temb table row
    Tensor r0, r1;                 // residual-phase sources (layer->R channels in total), at output resolution
    bool want_stats = false;       // emit per-channel statistics of the output (a GroupNorm will read it)
    bool out_f32_nchw = false;     // conv_out: write plan->io.out
    bool own_image = false;        // conv_small route with ONE tile per image (the producer normalises for its consumers)
    bool first_of_step = false;    // conv_in: advances the sampler's step index when the plan's pack_input launch is fused away
};

// the sizes every routing question is asked about: tensor (padded) channels of cat[x0, x1] and of cat[r0, r1], taps, output size
struct ConvShape {
    int Cin_t, R_t, taps, Wout, Hout;
};
inline ConvShape conv_shape(const ConvArgs& a) {
    return {a.x0.C + (a.x1.valid() ? a.x1.C : 0), (a.r0.valid() ? a.r0.C : 0) + (a.r1.valid() ? a.r1.C : 0),
            a.layer->ksize * a.layer->ksize, a.x0.W * a.up / a.stride, a.x0.H * a.up / a.stride};
}

// ---------------------------------------------------------------------------------------------------------------
// routing state: owned by plan.hip (which also holds its setters rldm_debug_set_flags / _set_flags2 / _force_tile / _timestamps)
// ---------------------------------------------------------------------------------------------------------------
int dbg_process();     // the process-wide routing word (rldm_debug_set_flags, enum rldm_flag; seeded by RLDM_DBG_FLAGS)
int dbg();             // ... | the options of the plan being built on this thread (Plan::flags)
int dbg2();            // second process-wide word (rldm_debug_set_flags2, enum rldm_flag2)

// in-kernel stamps (rldm_debug_timestamps, RLDM_ABLATE builds) of the launches the timeline tools pick, read once: RLDM_TS_TRUNK = n
// the persistent launch of n phases (RLDM_TS_TRUNK_FIRST: only the first one built), RLDM_TS_ORD = n conv n of a network,
// RLDM_TS_ATTN_L = L the attention launch of L tokens (AttnQkvParams::ts_L); none set: every conv and attention launch
struct StampEnv {
    const char *trunk, *trunk_first, *attn_l, *ord;
};
const StampEnv& stamp_env();
enum class StampSite { Conv, Attn, TestAttn, Trunk };
// where a launch writes its stamps (g_ts_buf or nowhere); n: the conv's ordinal (Conv), the launch's phase count (Trunk)
unsigned long long* stamp_buf(StampSite site, int n = 0);

// Producer-side GroupNorm: which convs write a normalised (+ activated) copy of their output for which
// consuming GroupNorm.  Filled by a recording pass over the network walk (the walk is the same in every pass, so a conv is
// identified by its ordinal), read by the sizing and the real pass.
struct ViewPlan {
    struct Part { int prod; int ch_off; };
    struct Cons {
        std::vector<Part> parts;
        int Ctot = 0, silu = 0, groups = 32;
        float eps = 1e-5f;
        bool ok = false;               // the consumer can read a pre-activated tensor (conv_small 3x3, fused attention)
        bool use = false;              // decided: ok and every part's producer can emit
    };
    struct Emit { const NormParams* norm; int ch_off; int Ctot; int silu; int groups; float eps; };
    std::vector<char> can_emit;        // by conv ordinal
    std::vector<int> out_c;            // output channels, by conv ordinal (tuning aid below)
    std::map<const NormParams*, Cons> cons;
    std::map<int, std::vector<Emit>> emit;
    void decide();
};

struct Builder {
    Plan* plan;
    bool dry;
    Arena arena;
    int next_id = 0;
    std::map<int, int> refs;
    std::map<int, Tensor> live;
    char* base = nullptr;
    int launches = 0;
    int temb_ld = 0;               // row stride of the time-embedding table (0: network has none)
    int* ticket_ptr = nullptr;     // split-K arrival counters (plan->tickets, zeroed at allocation; null in the dry pass)
    int tickets = 0;
    ViewPlan* vp = nullptr;        // producer-side GroupNorm plan (null: off)
    bool recording = false;        // the pass that fills *vp (a dry pass)
    int conv_ord = 0;
    int groups_hint = 32;
    std::map<const NormParams*, Tensor> view_tensors;      // consumer norm -> its pre-activated input (alive until consumed)
    const std::vector<ViewPlan::Emit>* cur_emit = nullptr; // of the conv being built
    int concurrent_plans = 1;      // the plan will share the device with this many of its kind (a sampler's chains)

    // recording pass: GroupNorm `n` over cat[x0, x1] is consumed by something that could read a pre-activated tensor instead
    void record_consumer(const NormParams* n, const Tensor& x0, const Tensor& x1, int silu, bool ok, int groups, float eps);
    // sizing / real pass: the pre-activated input of the consumer that owns norm `n`, if the plan has one
    bool take_view(const NormParams* n, Tensor* v);

    Tensor make(int B, int W, int H, int C);
    void add_stats(Tensor& t, int P);
    void retain(const Tensor& t) { refs[t.id]++; }
    void release(const Tensor& t);
    // ---- persistent trunk (trunk.hip): consecutive image-owning conv_small launches collected into one launch ----------------
    struct PendingTrunk {
        std::vector<TrunkPhase> phases;
        std::vector<Op> standalone;   // the same layers as launches of their own (a one-phase segment runs as that: a phase costs its
                                      // record fetch, the padded grid and the arrive for nothing)
        size_t lds = 0;
        int B = 0, ranks = 0;
        int ntile_n = 0, nwn = 1;      // channel tiles per image, 32-channel tiles per workgroup (multi-tile clusters: nwn == 2)
        int variant = 0;               // TrunkParams::variant
        double flops = 0, bytes = 0;
    } pend;
    bool trunk_open = false;
    std::map<int, int> trunk_seen;  // persistent launches built so far, by phase count (RLDM_TS_TRUNK_FIRST)
    std::vector<Tensor> deferred;  // releases held back while a segment is open (clusters of different images drift apart)
    // RLDM_FLAG_NO_PERSISTENT keeps every phase a launch of its own with the tiles unchanged (tests: identical results)
    static bool trunk_enabled() { return !(dbg() & RLDM_FLAG_NO_PERSISTENT); }
    void note_launch() {           // every launch that is not a trunk phase closes the open segment
        flush_trunk();
        ++launches;
    }
    int flush_trunk();

    // attention core as a trunk phase: x arrives normalised, C / 8 heads split over N / 32 = C / 32 workgroups of 8 waves
    static size_t trunk_attention_lds(int L, int C, int HG) { return attention_qkv2_lds_bytes(L, C, HG, 8); }
    bool trunk_attention_ok(const Tensor& x, bool pre) const;
    int cluster_attention_ranks(const Tensor& x, bool pre) const;       // ... of a multi-tile cluster; 0: not eligible
    static int device_cus();
    // a persistent launch spin-waits on its own workgroups: ALL of them must be resident at once, whatever else the plan's owner runs
    // beside it -- a sampler's other chains (concurrent_plans: two 256-workgroup launches could each hold part of the chip and wait
    // for the rest) and the device's real CU count (partitions / smaller parts)
    // (per_cu = 2: the 4-wave conv_stream variant, whose workgroups are built for two per CU)
    bool trunk_grid_fits(int ranks, int B, int per_cu = 1) const {
        return 8 * ranks * ((B + 7) / 8) * std::max(1, concurrent_plans) <= device_cus() * per_cu;
    }
    int own_tile_channels(int B, int npix, int N) const;
    void trunk_begin(int B, int ranks, int ntile_n = 0, int nwn = 1, int variant = -1);
    // multi-tile clusters (trunk.hip, kinds 8..13): an image = (N / 64) channel tiles x (pixels / 64) pixel tiles of conv_small's
    // 64 x 64 instance, all of them resident at once and on one XCD (8 * ranks * ceil(B / 8) workgroups <= the chip's CUs).
    // RLDM_FLAG_NO_CLUSTERS keeps these levels as separate launches
    // (and only for plans that run ALONE on the device: a 256-workgroup launch of one sampler chain and one of another could each
    //  hold part of the chip and wait for the rest -- sampler_build_plans passes its number of chains as concurrent_plans)
    bool cluster_enabled() const { return trunk_enabled() && !(dbg() & RLDM_FLAG_NO_CLUSTERS) && concurrent_plans <= 1; }
    int cluster_ranks(int B, int C, int npix) const;
    void trunk_push_attention(const AttnQkvParams& ap, double fl, double by);

    template <class T> T* ptr(size_t off) const { return reinterpret_cast<T*>(base + off); }
    bf16_t* tptr(const Tensor& t) const { return t.valid() ? ptr<bf16_t>(t.off) : nullptr; }
    const float2* sptr(const Tensor& t) const { return (t.valid() && t.P) ? ptr<float2>(t.st_off) : nullptr; }

    int gn_stats(Tensor& x);      // statistics of a tensor that did not come out of a conv epilogue (the test entry points' inputs)

    // ---- convs (plan.hip): conv_route asks each route's *_params in turn; the first that admits the conv has filled its ConvParams
    int conv(const ConvArgs& a0, Tensor* out);      // y = conv(...); consumes nothing (callers release inputs)
    int conv_route(const ConvArgs& a, const ConvShape& s, Tensor* out);
    static void conv_geometry(const ConvArgs& a, const ConvShape& s, int TW, int TH, int thv, ConvParams* q);
    // the kernels' *_supported shape checks look at WHICH pointers are set, not where they point: ask with stand-ins
    template <class F> static bool supported_with(ConvParams q, bool gn, bool f32_out, F&& supported) {
        if (gn) q.st0 = reinterpret_cast<const float2*>(&q);
        if (f32_out) q.y_nchw = reinterpret_cast<float*>(&q);
        return supported(q);
    }
    int require_gn_input(const ConvArgs& a, int Cin_t) const;
    void bind_conv(ConvParams& p, const ConvArgs& a, const ConvLayer::Packed& pk, const Tensor& y) const;
    // a launch of the plan, or (in_phase) the stand-alone form of a phase of the open persistent segment
    void emit(Op op, bool in_phase = false) { (in_phase ? pend.standalone : plan->ops).push_back(std::move(op)); }
    static void small_tile(int bm, int Wout, int Hout, int* tw, int* th);
    static bool small_params(const ConvArgs& a, const ConvShape& s, ConvParams* q, bool* epi_res);
    static int small_bn(const ConvParams& q, int taps, bool gn_fused, bool own = false);
    static bool small_gn_fused(const ConvArgs& a, int taps);
    static bool small_route(const ConvArgs& a, const ConvShape& s, ConvParams* q, bool* epi_res, int* bn);
    static bool small_route(const ConvArgs& a, const ConvShape& s);
    int conv_small(const ConvArgs& a, const ConvShape& s, ConvParams p, bool epi_res, int BN, Tensor* out);
    static constexpr int kSubMinBlocks = 96;
    static constexpr long long kAnyGrid = 1ll << 40;
    static bool stream_params_tw(const ConvArgs& a, const ConvShape& s, StreamInst inst, long long min_blocks, long long max_blocks,
                                 ConvParams* q, StreamTile tile = {});
    static bool stream_params(const ConvArgs& a, const ConvShape& s, ConvParams* q);
    int conv_stream(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out);
    static bool c16_params(const ConvArgs& a, const ConvShape& s, ConvParams* q);
    int conv_c16(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out);
    static bool o4_params(const ConvArgs& a, const ConvShape& s, ConvParams* q);
    int conv_o4(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out);
    static bool ds2_params(const ConvArgs& a, const ConvShape& s, ConvParams* q);
    int conv_ds2(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out);
    static bool regw_params(const ConvArgs& a, const ConvShape& s, ConvParams* q);
    int conv_regw(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out);
    static constexpr int kFoldAboveP = 32;
    int fold_stats(Tensor& y);
    int conv_generic(const ConvArgs& a, const ConvShape& s, Tensor* out);
};

// Two passes over the same walk: a dry one sizes the activation arena (and the split-K counters), the real one bakes
// device pointers into the launch list.
// (count_only: the recording and sizing passes alone -- *launches is the result, the plan gets no arena and no ops)
int build_plan(Plan* plan, int temb_ld, const std::function<int(Builder&)>& walk, int* launches = nullptr, int concurrent_plans = 1,
               bool count_only = false);

// ---------------------------------------------------------------------------------------------------------------
// what the sampler (sampler.hip) and the test entry points share
// ---------------------------------------------------------------------------------------------------------------
// SchedParams / SchedFuse::mode of a scheduler step (sched_prev) from RLDM_SAMPLER_* and RLDM_PRED_*; -1 for RLDM_SAMPLER_UNIPC, whose
// rows are 12 wide and run through sched_unipc_kernel alone
int sched_mode_word(int sampler_mode, int prediction_type);
// where a scheduler step reads its noise: the tensor (offset to the first sample) and the elements between two steps' rows
struct NoiseSrc {
    const float* p;
    long long step_stride;
};
// the fixed part of a fused tail (the scheduler step in conv_out's epilogue): table, step word, x, x_prev, mode, noise source and --
// pack != null -- the next step's conv_in input
void fill_sched_fuse(SchedFuse& f, const float* coef_table, const int* step_ptr, const float* x, float* x_prev, int mode,
                     NoiseSrc noise, bf16_t* pack, int pack_ld);

struct NetCommon;
}  // namespace rldm

// ---- the model objects behind the C handles (runtime.hip) ------------------------------------------------------
struct rldm_unet {
    rldm_unet_config cfg;
    rldm::ParamStore params;
    std::unique_ptr<rldm::NetCommon> net;           // the layers and their walks (runtime.hip; never null)
    int temb_dim = 0;                               // time_embed_dim
    rldm::DevBuf w1, b1, w2, b2, wp, bp;            // fp32 time-embedding weights
    std::map<int, std::unique_ptr<rldm::Plan>> plans;   // per batch size
    rldm::DevBuf t_dev, temb_tab;                   // scratch for rldm_unet_forward
    rldm::DevBuf temb_scratch;                      // hidden layers of the time-embedding MLP (launch_temb)
    uint64_t generation = 0;                        // bumped whenever the device weights are (re)built: samplers re-plan
    int temb_rows_cap = 0;
    int plan_flags = 0;                             // rldm_unet_set_plan_flags: routing options of the rldm_unet_forward plans
    std::map<int, bool> trunk_checked;              // batch -> the plan's persistent launches passed their self-check once
    std::vector<std::string> resnet_order;

    int levels() const { return cfg.num_levels; }
    rldm_unet();
    ~rldm_unet();
};

struct rldm_vae {
    uint64_t generation = 0;                        // see rldm_unet::generation
    rldm_vae_config cfg;
    rldm::ParamStore params;
    std::unique_ptr<rldm::NetCommon> net;           // the layers and their walks (runtime.hip; never null)
    struct Key { int B, w, h, enc; bool operator<(const Key& o) const { return std::tie(B, w, h, enc) < std::tie(o.B, o.w, o.h, o.enc); } };
    std::map<Key, std::unique_ptr<rldm::Plan>> plans;
    rldm_vae();
    ~rldm_vae();
};

namespace rldm {
// concurrent_plans: how many plans of this kind will run side by side (a sampler's chains)
int unet_make_plan(rldm_unet* m, int B, std::unique_ptr<Plan>* out, int* launches = nullptr, int flags = 0, int concurrent_plans = 1);
int unet_temb_ld(const rldm_unet* m);       // row length of the time-embedding table
int unet_temb_off(const rldm_unet* m, const std::string& resnet_prefix);   // that resnet's first column in a row, or -1
// time-embedding table for `rows` timesteps (host floats) into `tab`
int unet_temb(rldm_unet* m, const float* t_dev, int rows, float* tab, hipStream_t s);
int vae_make_plan(rldm_vae* m, int B, int w, int h, bool enc, std::unique_ptr<Plan>* out, int flags = 0);
}  // namespace rldm
