// Kernel-level test and bench entry points: one conv, one attention launch or one attention block as a plan of its own.
#include "runtime.h"

using namespace rldm;

namespace {
// the synthetic operands' generator: uniform in [-1, 1) from a linear congruential sequence
struct Lcg {
    uint32_t state;
    explicit Lcg(uint32_t seed) : state(seed) {}
    float operator()() {
        state = state * 1664525u + 1013904223u;
        return ((state >> 8) & 0xffff) / 32768.0f - 1.0f;
    }
};

// average time of `unit` over `iters` runs on `st`, between a HIP event pair
int timed_loop(hipStream_t st, int iters, const std::function<int()>& unit, float* avg_us) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int rc = [&]() -> int {
        RLDM_HIP_CHECK(hipEventCreate(&e0));
        RLDM_HIP_CHECK(hipEventCreate(&e1));
        RLDM_HIP_CHECK(hipEventRecord(e0, st));
        for (int i = 0; i < iters; ++i)
            if (unit()) return 1;
        RLDM_HIP_CHECK(hipEventRecord(e1, st));
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        float ms = 0.f;
        RLDM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = ms * 1000.0f / iters;
        return 0;
    }();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// a conv output's statistics partials [B][P][C] (device) summed over P into hs: image b's C (sum, sumsq) pairs start at hs[b * ld]
int sum_partials(const void* part_dev, int B, int P, int C, float* hs, size_t ld) {
    std::vector<float2> part((size_t)B * P * C);
    RLDM_HIP_CHECK(hipMemcpy(part.data(), part_dev, part.size() * sizeof(float2), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < P; ++q)
            for (int c = 0; c < C; ++c) {
                const float2 v = part[((size_t)b * P + q) * C + c];
                hs[b * ld + (size_t)c * 2] += v.x;
                hs[b * ld + (size_t)c * 2 + 1] += v.y;
            }
    return 0;
}

// n device floats as host bf16, each through pre(index, value) before the rounding
template <class Pre> int download_as_bf16(const float* dev, size_t n, std::vector<bf16_t>& hb, Pre&& pre) {
    std::vector<float> h(n);
    RLDM_HIP_CHECK(hipMemcpy(h.data(), dev, n * 4, hipMemcpyDeviceToHost));
    hb.resize(n);
    for (size_t i = 0; i < n; ++i) hb[i] = f32_to_bf16(pre(i, h[i]));
    return 0;
}
int download_as_bf16(const float* dev, size_t n, std::vector<bf16_t>& hb) {
    return download_as_bf16(dev, n, hb, [](size_t, float v) { return v; });
}
int upload_bf16_as_f32(const std::vector<bf16_t>& hb, float* dev) {
    std::vector<float> h(hb.size());
    for (size_t i = 0; i < hb.size(); ++i) h[i] = bf16_to_f32(hb[i]);
    RLDM_HIP_CHECK(hipMemcpy(dev, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
}  // namespace

extern "C" {

// ---- kernel-level test entry points ---------------------------------------------------------------------------------
namespace {
struct ConvCase {
    Layers layers;
    Plan plan;
    Tensor t0, t1, tr, out;
    int Wout = 0, Hout = 0, C0p = 0;
};
// one fused conv as a plan: [statistics of x0/x1 when gn] + conv
int make_conv_case(ConvCase& cc, const rldm_conv_desc* d, const float* weight, const float* bias, const float* gamma,
                   const float* beta, int res_channels, bool with_temb, bool output_layer = false) {
    const bool with_res = res_channels > 0;
    const int Cin = d->Cin0 + d->Cin1;
    cc.C0p = d->Cin1 ? d->Cin0 : pad16(d->Cin0);
    RLDM_REQUIRE(d->Cin1 == 0 || (d->Cin0 % 16 == 0 && Cin % 16 == 0), "concat test needs Cin0 % 16 == 0 and Cin % 16 == 0");
    ParamStore ps;
    ps.host["c.weight"].assign(weight, weight + (size_t)d->Cout * Cin * d->ksize * d->ksize);
    ps.host["c.bias"].assign(bias, bias + d->Cout);
    if (cc.layers.add_conv(ps, "c", d->Cout, Cin, d->ksize)) return 1;
    if (with_res) {                                   // `+ res`: identity residual phase over Cout channels, or (bench
        ConvLayer* L = cc.layers.get_conv("c");       // only) a synthetic 1x1 shortcut over res_channels
        L->R = res_channels;
        L->sc_identity = res_channels == d->Cout;
        if (!L->sc_identity) {
            L->sc_w.resize((size_t)d->Cout * res_channels);
            Lcg rnd(777u);
            for (auto& v : L->sc_w) v = rnd() / std::sqrt((float)res_channels);
        }
    }
    if (d->gn) {
        RLDM_REQUIRE(gamma && beta && cc.C0p + d->Cin1 == Cin, "GroupNorm test needs unpadded channels");
        ps.host["n.weight"].assign(gamma, gamma + Cin);
        ps.host["n.bias"].assign(beta, beta + Cin);
        if (cc.layers.add_norm(ps, "n", Cin)) return 1;
    }
    const int s = d->stride, up = d->upsample ? 2 : 1;
    cc.Wout = d->Win * up / s;
    cc.Hout = d->Hin * up / s;
    RLDM_REQUIRE(!output_layer || (d->Cout <= 4 && !with_res && !with_temb), "an output layer has <= 4 channels, no residual, no time embedding");
    auto walk = [&cc, d, with_res, res_channels, with_temb, output_layer, s, up](Builder& bb) -> int {
        cc.t0 = bb.make(d->B, d->Win, d->Hin, cc.C0p);
        cc.t1 = Tensor();
        cc.tr = Tensor();
        if (d->Cin1) cc.t1 = bb.make(d->B, d->Win, d->Hin, d->Cin1);
        if (with_res) cc.tr = bb.make(d->B, cc.Wout, cc.Hout, res_channels);
        if (d->gn) {
            if (bb.gn_stats(cc.t0)) return 1;
            if (d->Cin1 && bb.gn_stats(cc.t1)) return 1;
        }
        ConvArgs a;
        a.layer = cc.layers.get_conv("c");
        a.x0 = cc.t0; a.x1 = cc.t1;
        a.stride = s; a.pad_mode = d->pad_mode; a.up = up;
        a.gn = d->gn ? cc.layers.get_norm("n") : nullptr;
        a.eps = d->eps; a.silu = d->silu;
        a.temb_off = with_temb ? 0 : -1;
        a.r0 = cc.tr;
        a.want_stats = true;
        // RLDM_FLAG2_FP32_OUT: a conv of <= 4 output channels is a network OUTPUT layer -- fp32 NCHW into plan.io.out (the VAE
        // decoder's conv_out), no bf16 tensor, no statistics
        if (output_layer || ((dbg2() & RLDM_FLAG2_FP32_OUT) && d->Cout <= 4 && !with_res && !with_temb)) {
            a.out_f32_nchw = true;
            a.want_stats = false;
        }
        return bb.conv(a, &cc.out);
    };
    return build_plan(&cc.plan, d->Cout, walk);
}
}  // namespace

int rldm_test_conv(const rldm_conv_desc* d, const float* x0, const float* x1, const float* weight, const float* bias,
                   const float* gamma, const float* beta, const float* temb, const float* res, float* y, void* stream) {
    RLDM_REQUIRE(d && x0 && weight && bias && y, "null argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ConvCase cc;
    if (make_conv_case(cc, d, weight, bias, gamma, beta, res ? d->Cout : 0, temb != nullptr)) return 1;
    DevBuf tembd;
    if (temb && upload(tembd, temb, (size_t)d->B * d->Cout * 4)) return 1;
    char* base = cc.plan.arena.as<char>();
    auto tp = [&](const Tensor& t) { return reinterpret_cast<bf16_t*>(base + t.off); };
    if (launch_nchw_f32_to_nhwc_bf16(x0, tp(cc.t0), d->B, d->Cin0, d->Win, d->Hin, cc.C0p, st)) return 1;
    if (d->Cin1 && launch_nchw_f32_to_nhwc_bf16(x1, tp(cc.t1), d->B, d->Cin1, d->Win, d->Hin, d->Cin1, st)) return 1;
    if (res && launch_nchw_f32_to_nhwc_bf16(res, tp(cc.tr), d->B, d->Cout, cc.Wout, cc.Hout, d->Cout, st)) return 1;
    cc.plan.io.temb = tembd.as<float>();
    cc.plan.io.temb_rows_per_step = d->B;
    cc.plan.io.temb_per_sample = 1;
    if (!cc.out.valid()) cc.plan.io.out = y;         // (an output layer: fp32 NCHW straight into the caller's buffer)
    if (cc.plan.run(st)) return 1;
    if (cc.out.valid() && launch_nhwc_bf16_to_nchw_f32(tp(cc.out), y, d->B, d->Cout, cc.Wout, cc.Hout, d->Cout, st)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// per-channel statistics the conv epilogue emitted for its output: (sum, sumsq) over each image -> stats [B][Cout][2]
int rldm_test_conv_stats(const rldm_conv_desc* d, const float* x0, const float* weight, const float* bias, float* stats,
                         void* stream) {
    RLDM_REQUIRE(d && x0 && weight && bias && stats, "null argument");
    RLDM_REQUIRE(d->Cin1 == 0 && !d->gn, "stats test: plain single-input conv only");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ConvCase cc;
    if (make_conv_case(cc, d, weight, bias, nullptr, nullptr, 0, false)) return 1;
    char* base = cc.plan.arena.as<char>();
    if (launch_nchw_f32_to_nhwc_bf16(x0, reinterpret_cast<bf16_t*>(base + cc.t0.off), d->B, d->Cin0, d->Win, d->Hin, cc.C0p, st)) return 1;
    if (cc.plan.run(st)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_REQUIRE(cc.out.P > 0, "internal: conv output carries no statistics");
    std::vector<float> hs((size_t)d->B * d->Cout * 2, 0.f);
    if (sum_partials(base + cc.out.st_off, d->B, cc.out.P, d->Cout, hs.data(), (size_t)d->Cout * 2)) return 1;
    RLDM_HIP_CHECK(hipMemcpy(stats, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// the scheduler step in the output layer's epilogue, as a sampler's fused tail runs it (sampler_build_plans)
int rldm_test_conv_sched(const rldm_conv_desc* d, const float* x0, const float* weight, const float* bias, const float* gamma,
                         const float* beta, const rldm_conv_sched_desc* sch, float* eps, char* op_name, size_t name_cap, void* stream) {
    RLDM_REQUIRE(d && x0 && weight && bias && sch && eps && op_name && name_cap > 0, "null argument");
    RLDM_REQUIRE(d->Cin1 == 0 && d->Cout >= 1 && d->Cout <= 4, "sched test: single-input conv of <= 4 output channels only");
    RLDM_REQUIRE(sch->sampler_mode >= RLDM_SAMPLER_DDIM && sch->sampler_mode <= RLDM_SAMPLER_DPMSOLVER, "unknown sampler mode");
    RLDM_REQUIRE(sch->prediction_type >= RLDM_PRED_EPSILON && sch->prediction_type <= RLDM_PRED_SAMPLE, "unknown prediction type");
    RLDM_REQUIRE(sch->coef_table && sch->step && sch->x && sch->x_prev, "null argument");
    RLDM_REQUIRE(sch->sampler_mode != RLDM_SAMPLER_DPMSOLVER || sch->noise != nullptr, "multistep mode needs the x0 history");
    RLDM_REQUIRE(!sch->pack || sch->pack_ld >= d->Cout, "pack_ld below the output channels");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ConvCase cc;
    if (make_conv_case(cc, d, weight, bias, gamma, beta, 0, false, true)) return 1;
    RLDM_REQUIRE(!cc.out.valid() && !cc.plan.ops.empty(), "internal: the output layer was not built as one");
    char* base = cc.plan.arena.as<char>();
    if (launch_nchw_f32_to_nhwc_bf16(x0, reinterpret_cast<bf16_t*>(base + cc.t0.off), d->B, d->Cin0, d->Win, d->Hin, cc.C0p, st)) return 1;
    PlanIO& io = cc.plan.io;
    io.out = eps;
    fill_sched_fuse(io.sch, sch->coef_table, sch->step, sch->x, sch->x_prev, sched_mode_word(sch->sampler_mode, sch->prediction_type),
                    {sch->noise, sch->noise_step_stride}, reinterpret_cast<bf16_t*>(sch->pack), sch->pack_ld);
    if (cc.plan.run(st)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    const std::string& name = cc.plan.ops.back().name;       // (the conv is the plan's last launch: an output layer emits no statistics to fold)
    RLDM_REQUIRE(name.size() + 1 <= name_cap, "op name buffer too small");
    memcpy(op_name, name.c_str(), name.size() + 1);
    return 0;
}

// times the fused conv kernel alone (HIP events on `stream`) on synthetic device data; the statistics launches of a
// GroupNorm case run once before the timed region
int rldm_bench_conv(const rldm_conv_desc* d, int with_res, int with_temb, int warmup, int iters, float* avg_us,
                    char* kernel_name, size_t name_cap, void* stream) {
    RLDM_REQUIRE(d && avg_us && iters >= 1, "bad argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int Cin = d->Cin0 + d->Cin1;
    const int taps = d->ksize * d->ksize;
    std::vector<float> w((size_t)d->Cout * Cin * taps), bias(d->Cout), gamma(Cin, 1.f), beta(Cin, 0.f);
    Lcg rnd(12345u);
    const float ws = 1.0f / std::sqrt((float)Cin * taps);
    for (auto& v : w) v = rnd() * ws;
    for (auto& v : bias) v = rnd() * 0.1f;
    ConvCase cc;
    if (make_conv_case(cc, d, w.data(), bias.data(), gamma.data(), beta.data(), with_res, with_temb != 0)) return 1;
    DevBuf tembd;
    if (with_temb) {
        std::vector<float> t((size_t)d->B * d->Cout);
        for (auto& v : t) v = rnd();
        if (upload(tembd, t.data(), t.size() * 4)) return 1;
    }
    {   // synthetic activations: bf16 uniform(-1, 1)
        std::vector<bf16_t> h(cc.plan.arena.bytes / 2);
        for (auto& v : h) v = f32_to_bf16(rnd());
        RLDM_HIP_CHECK(hipMemcpy(cc.plan.arena.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    cc.plan.io.temb = tembd.as<float>();
    cc.plan.io.temb_rows_per_step = d->B;
    cc.plan.io.temb_per_sample = 1;
    DevBuf outd;
    if (!cc.out.valid()) {
        if (outd.alloc((size_t)d->B * d->Cout * cc.Wout * cc.Hout * sizeof(float))) return 1;
        cc.plan.io.out = outd.as<float>();
    }
    RLDM_REQUIRE(!cc.plan.ops.empty(), "internal: empty plan");
    // the timed unit: the conv launch, plus the GroupNorm+SiLU launch in front of it on the conv_small.hip route
    size_t last = cc.plan.ops.size() - 1;           // the conv itself: the last op whose name starts with "conv_" (a gn_fold of
    while (last > 0 && cc.plan.ops[last].name.rfind("conv_", 0) != 0) --last;      // its output statistics may follow it)
    size_t first = last;
    if (first > 0 && cc.plan.ops[first - 1].name == "gn_apply_kernel") --first;
    auto run_unit = [&]() {
        for (size_t o = first; o <= last; ++o)
            if (cc.plan.ops[o].fn(st)) return 1;
        return 0;
    };
    if (kernel_name && name_cap) {
        const std::string nm = (first < last ? "gn_apply+" : "") + cc.plan.ops[last].name;
        strncpy(kernel_name, nm.c_str(), name_cap - 1);
        kernel_name[name_cap - 1] = 0;
    }
    if (cc.plan.run(st)) return 1;
    for (int i = 0; i < warmup; ++i)
        if (run_unit()) return 1;
    return timed_loop(st, iters, run_unit, avg_us);
}

// the time-embedding table of n timesteps, through the conversion and the call rldm_unet_forward and the samplers make
int rldm_test_temb(rldm_unet* m, const int64_t* timesteps, int n, float* table, void* stream) {
    RLDM_REQUIRE(m && timesteps && table && n >= 1, "bad argument");
    RLDM_REQUIRE(m->params.finalized, "rldm_unet_finalize has not been called");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<float> tf(n);
    for (int i = 0; i < n; ++i) tf[i] = (float)timesteps[i];
    DevBuf td;
    if (upload(td, tf.data(), (size_t)n * 4)) return 1;
    if (unet_temb(m, td.as<float>(), n, table, st)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int rldm_test_temb_layout(rldm_unet* m, const char* resnet_prefix, int* value) {
    RLDM_REQUIRE(m && value, "null argument");
    RLDM_REQUIRE(m->params.finalized, "rldm_unet_finalize has not been called");
    *value = resnet_prefix ? unet_temb_off(m, resnet_prefix) : unet_temb_ld(m);
    RLDM_REQUIRE(*value >= 0, std::string("no resnet '") + resnet_prefix + "' with a time-embedding projection");
    return 0;
}

int rldm_test_attention(const float* qkv, int B, int L, int C, float* out, void* stream) {
    RLDM_REQUIRE(qkv && out, "null argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // host-side conversion keeps this test path trivial: qkv [B][L][3C] bf16 with q pre-scaled by log2(e)/sqrt(8)
    std::vector<bf16_t> hq;
    const float qs = attn_q_scale(8);
    if (download_as_bf16(qkv, (size_t)B * L * 3 * C, hq, [&](size_t i, float v) { return (int)(i % (3 * (size_t)C)) < C ? v * qs : v; })) return 1;
    DevBuf dq, dout;
    if (upload(dq, hq.data(), hq.size() * 2)) return 1;
    if (dout.alloc((size_t)B * L * C * 2)) return 1;
    AttnParams ap;
    ap.qkv = dq.as<bf16_t>(); ap.out = dout.as<bf16_t>();
    ap.B = B; ap.L = L; ap.C = C;
    if (launch_attention(ap, st)) return 1;
    std::vector<bf16_t> ho((size_t)B * L * C);
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_HIP_CHECK(hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost));
    return upload_bf16_as_f32(ho, out);
}

// The fused GroupNorm -> to_q/to_k/to_v -> softmax(q k^T / sqrt(8)) v launch on its own (what runs inside every
// attention block of the UNet): x device fp32 [B][L][C] (token-major), gamma/beta host [C], wqkv host [3C][C] (rows
// q | k | v, torch Linear layout), bqkv host [3C] -> out device fp32 [B][L][C] (heads concatenated, before to_out).
namespace {
struct AttnCase {
    DevBuf dx, dst, dg, dbt, dw, dbias, dout;
    AttnQkvParams ap;
};
// x_bf16 host [B][L][C]; builds the per-image statistics row, the per-head fragments and the launch parameters
int make_attn_case(AttnCase& ac, const std::vector<bf16_t>& hb, int B, int L, int C, int groups, float eps, const float* gamma,
                   const float* beta, const float* wqkv, const float* bqkv) {
    const size_t n = (size_t)B * L * C;
    std::vector<float> stats((size_t)B * C * 2, 0.f);      // one partial row per image: (sum, sum of squares) of the bf16 values
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            double S = 0.0, SS = 0.0;
            for (int l = 0; l < L; ++l) {
                const double v = bf16_to_f32(hb[((size_t)b * L + l) * C + c]);
                S += v;
                SS += v * v;
            }
            stats[((size_t)b * C + c) * 2] = (float)S;
            stats[((size_t)b * C + c) * 2 + 1] = (float)SS;
        }
    std::vector<float> w((size_t)3 * C * C), bb((size_t)3 * C);
    const float qs = attn_q_scale(8);
    for (size_t i = 0; i < w.size(); ++i) w[i] = wqkv[i] * (i < (size_t)C * C ? qs : 1.f);
    for (int i = 0; i < 3 * C; ++i) bb[i] = bqkv[i] * (i < C ? qs : 1.f);
    std::vector<bf16_t> img;
    std::vector<float> bias;
    pack_attn_head_frags(w.data(), bb.data(), C, img, bias);
    if (upload(ac.dx, hb.data(), n * 2) || upload(ac.dst, stats.data(), stats.size() * 4) || upload(ac.dg, gamma, C * 4) ||
        upload(ac.dbt, beta, C * 4) || upload(ac.dw, img.data(), img.size() * 2) || upload(ac.dbias, bias.data(), bias.size() * 4))
        return 1;
    if (ac.dout.alloc(n * 2)) return 1;
    AttnQkvParams& ap = ac.ap;
    memset(&ap, 0, sizeof(ap));
    ap.x = ac.dx.as<bf16_t>(); ap.st = ac.dst.as<float2>(); ap.P = 1;
    ap.gamma = ac.dg.as<float>(); ap.beta = ac.dbt.as<float>(); ap.eps = eps; ap.groups = groups;
    const int cpg = C / groups;
    ap.inv_n = (float)(1.0 / ((double)L * cpg));
    ap.magic_cpg = ((1 << 20) + cpg - 1) / cpg;
    ap.wfrag = ac.dw.as<bf16_t>(); ap.bias = ac.dbias.as<float>(); ap.out = ac.dout.as<bf16_t>();
    ap.B = B; ap.L = L; ap.C = C;
    ap.ts = stamp_buf(StampSite::TestAttn);                                                 // ABLATE builds: phase stamps (rldm_debug_timestamps)
    ap.ts_L = L;
    return 0;
}
}  // namespace

int rldm_test_attention_qkv(const float* x, int B, int L, int C, int groups, float eps, const float* gamma, const float* beta,
                            const float* wqkv, const float* bqkv, float* out, void* stream) {
    RLDM_REQUIRE(x && gamma && beta && wqkv && bqkv && out, "null argument");
    RLDM_REQUIRE(C % 16 == 0 && C % groups == 0, "attention_qkv: channels must be a multiple of 16 and of the group count");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * L * C;
    std::vector<bf16_t> hb;
    if (download_as_bf16(x, n, hb)) return 1;
    AttnCase ac;
    if (make_attn_case(ac, hb, B, L, C, groups, eps, gamma, beta, wqkv, bqkv)) return 1;
    if (launch_attention_qkv(ac.ap, st)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<bf16_t> ho(n);
    RLDM_HIP_CHECK(hipMemcpy(ho.data(), ac.dout.p, n * 2, hipMemcpyDeviceToHost));
    return upload_bf16_as_f32(ho, out);
}

int rldm_test_attention_route(int B, int L, int C, int* route) {
    RLDM_REQUIRE(route && B >= 1 && L >= 1 && C >= 8, "bad argument");
    attention_qkv_route(B, L, C, Builder::device_cus(), route);
    return 0;
}

// The attention block as the plan runs it: the fused launch, then the output projection y = x + to_out(o) with y's statistics
// partials, in one of three forms: 0 = launch_attention_proj behind the launch, 1 = the tail behind the seam inside the launch,
// 2 = the regular 1x1 conv (the unfused plan; stats: per-image totals in partial row 0, the other rows zero).
int rldm_test_attention_block(const float* x, int B, int L, int C, int groups, float eps, const float* gamma, const float* beta,
                              const float* wqkv, const float* bqkv, const float* wout, const float* bout, int mode, float* y,
                              float* stats, void* stream) {
    RLDM_REQUIRE(x && gamma && beta && wqkv && bqkv && wout && bout && y && stats, "null argument");
    RLDM_REQUIRE(mode >= 0 && mode <= 2 && C % 16 == 0 && C % groups == 0 && L % 64 == 0, "attention_block: bad argument");
    RLDM_REQUIRE(attention_proj_fusable(B, L, C, -1), "attention_block: the output projection cannot ride on this shape");
    RLDM_REQUIRE(mode != 1 || attention_proj_fusable(B, L, C, Builder::device_cus()),
                 "attention_block: not every workgroup of the launch is resident on this device (no seam)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * L * C;
    const int parts = L / 64;
    std::vector<bf16_t> hb;
    if (download_as_bf16(x, n, hb)) return 1;
    AttnCase ac;
    if (make_attn_case(ac, hb, B, L, C, groups, eps, gamma, beta, wqkv, bqkv)) return 1;
    std::vector<bf16_t> hy(n);
    std::vector<float> hs((size_t)B * parts * C * 2, 0.f);
    if (mode < 2) {
        // to_out in the tail's A-fragment order, as the plan packs it (NetCommon::attention): one k-group, no residual steps
        ConvLayer to_out;
        to_out.name = "to_out";
        to_out.Cout = to_out.Cin = C;
        to_out.ksize = 1;
        to_out.w.assign(wout, wout + (size_t)C * C);
        to_out.b.assign(bout, bout + C);
        ConvLayer::Packed* pk = nullptr;
        if (to_out.get_fragpacked(C, 32, 1, true, &pk)) return 1;
        DevBuf dy, dstats, dctr, derr;
        if (dy.alloc(n * 2) || dstats.alloc(hs.size() * 4) || dctr.alloc((size_t)B * 32 * 4) || derr.alloc(64)) return 1;
        RLDM_HIP_CHECK(hipMemset(dctr.p, 0, dctr.bytes));
        RLDM_HIP_CHECK(hipMemset(derr.p, 0, derr.bytes));
        AttnQkvParams& ap = ac.ap;
        ap.proj_w = pk->w.as<bf16_t>(); ap.proj_bias = pk->bias.as<float>(); ap.proj_res = ac.dx.as<bf16_t>();
        ap.proj_y = dy.as<bf16_t>(); ap.proj_stats = dstats.as<float2>();
        if (mode == 1) {
            ap.proj_counter = dctr.as<unsigned>();
            ap.proj_error = derr.as<int>();
            if (launch_attention_qkv(ap, st)) return 1;
        } else {
            AttnQkvParams plain = ap;
            plain.proj_w = nullptr;
            if (launch_attention_qkv(plain, st) || launch_attention_proj(ap, st)) return 1;
        }
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        int err = 0;
        RLDM_HIP_CHECK(hipMemcpy(&err, derr.p, 4, hipMemcpyDeviceToHost));
        RLDM_REQUIRE(err == 0, "attention_block: the seam reported error " + std::to_string(err) +
                                   " (1: a wait gave up, 2: an image's workgroups on several XCDs)");
        RLDM_HIP_CHECK(hipMemcpy(hy.data(), dy.p, n * 2, hipMemcpyDeviceToHost));
        RLDM_HIP_CHECK(hipMemcpy(hs.data(), dstats.p, hs.size() * 4, hipMemcpyDeviceToHost));
    } else {
        if (launch_attention_qkv(ac.ap, st)) return 1;
        rldm_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.B = B; d.Cin0 = C; d.Win = L / 8; d.Hin = 8; d.Cout = C; d.ksize = 1; d.stride = 1; d.eps = eps;
        ConvCase cc;
        if (make_conv_case(cc, &d, wout, bout, nullptr, nullptr, C, false)) return 1;
        char* base = cc.plan.arena.as<char>();
        RLDM_HIP_CHECK(hipMemcpyAsync(base + cc.t0.off, ac.dout.p, n * 2, hipMemcpyDeviceToDevice, st));
        RLDM_HIP_CHECK(hipMemcpyAsync(base + cc.tr.off, ac.dx.p, n * 2, hipMemcpyDeviceToDevice, st));
        if (cc.plan.run(st)) return 1;
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        RLDM_REQUIRE(cc.out.P > 0, "internal: conv output carries no statistics");
        RLDM_HIP_CHECK(hipMemcpy(hy.data(), base + cc.out.off, n * 2, hipMemcpyDeviceToHost));
        if (sum_partials(base + cc.out.st_off, B, cc.out.P, C, hs.data(), (size_t)parts * C * 2)) return 1;
    }
    RLDM_HIP_CHECK(hipMemcpy(stats, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    return upload_bf16_as_f32(hy, y);
}

// times the fused attention launch alone (HIP events on `stream`) on synthetic data of the given geometry
int rldm_bench_attention_qkv(int B, int L, int C, int warmup, int iters, float* avg_us, void* stream) {
    RLDM_REQUIRE(avg_us && iters >= 1 && C % 32 == 0, "bad argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * L * C;
    Lcg rnd(4242u);
    std::vector<bf16_t> hb(n);
    for (auto& v : hb) v = f32_to_bf16(rnd() * 1.7f + 0.2f);
    std::vector<float> gamma(C, 1.f), beta(C, 0.f), w((size_t)3 * C * C), bb((size_t)3 * C, 0.f);
    const float ws = 2.0f / std::sqrt((float)C);
    for (auto& v : w) v = rnd() * ws;
    AttnCase ac;
    if (make_attn_case(ac, hb, B, L, C, 32, 1e-5f, gamma.data(), beta.data(), w.data(), bb.data())) return 1;
    for (int i = 0; i < warmup; ++i)
        if (launch_attention_qkv(ac.ap, st)) return 1;
    return timed_loop(st, iters, [&]() { return launch_attention_qkv(ac.ap, st); }, avg_us);
}

}  // extern "C"
