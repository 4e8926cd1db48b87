// The plan builder: which kernel instance, tile and route every conv of a network walk runs on (choose_tile, Builder), the three
// passes that turn a walk into a Plan (build_plan), how a Plan runs -- and the routing state those decisions read, with its setters.
#include "runtime.h"

namespace rldm {

// routing switches (rldm_debug_set_flags, enum rldm_flag); RLDM_DBG_FLAGS seeds them for runs of unmodified drivers
static int g_dbg_flags = getenv("RLDM_DBG_FLAGS") ? atoi(getenv("RLDM_DBG_FLAGS")) : 0;
// ... and the options of the plan being built (Plan::flags: rldm_sampler_config::plan_flags, rldm_unet_set_plan_flags, the fall-back
// of a sampler whose persistent launches failed their self-check) -- scoped to that plan, unlike the process-wide word above
static thread_local int t_plan_flags = 0;
int dbg_process() { return g_dbg_flags; }
int dbg() { return g_dbg_flags | t_plan_flags; }
// second word of process-wide routing switches (rldm_debug_set_flags2, enum rldm_flag2)
static int g_dbg_flags2 = 0;
int dbg2() { return g_dbg_flags2; }
// ConvParams::dbg: the kernels' ablation bits.  The routing word reaches them only in RLDM_ABLATE builds (the timeline tools).
static inline int kernel_dbg() {
#ifdef RLDM_ABLATE
    return dbg();
#else
    return 0;
#endif
}
static unsigned long long* g_ts_buf = nullptr;   // rldm_debug_timestamps: device [4][64] s_memtime stamps
const StampEnv& stamp_env() {
    static const StampEnv e = {getenv("RLDM_TS_TRUNK"), getenv("RLDM_TS_TRUNK_FIRST"), getenv("RLDM_TS_ATTN_L"), getenv("RLDM_TS_ORD")};
    return e;
}
unsigned long long* stamp_buf(StampSite site, int n) {
    const StampEnv& e = stamp_env();
    switch (site) {
        case StampSite::Conv:     return e.ord ? (atoi(e.ord) == n ? g_ts_buf : nullptr) : (e.attn_l || e.trunk) ? nullptr : g_ts_buf;
        case StampSite::Attn:     return (e.trunk || e.ord) ? nullptr : g_ts_buf;
        case StampSite::TestAttn: return e.trunk ? nullptr : g_ts_buf;
        case StampSite::Trunk:    return (e.trunk && atoi(e.trunk) == n) ? g_ts_buf : nullptr;
    }
    return nullptr;
}
static constexpr int kInst4MinBlocks = 96;      // (192 -> 96: nuScenes at 4 images 87.4 -> 89.4, KITTI at 8 images 134.4 -> 137.5 img/s)
static int g_force_bm = 0, g_force_bn = 0, g_force_ks = 0;     // rldm_debug_force_tile: tuning override (0: automatic)

struct PlanFlagScope {            // t_plan_flags = the plan's options for the duration of its construction
    int saved;
    explicit PlanFlagScope(int f) : saved(t_plan_flags) { t_plan_flags = f; }
    ~PlanFlagScope() { t_plan_flags = saved; }
};

// algorithmic FLOPs (2*MACs; an identity residual multiplies nothing) and HBM bytes (input, weights, `out_copies` outputs,
// residual sources -- each touched once) of a conv.  `res_weights`: the kernel reads the residual phase's weights
static double conv_flops(const ConvArgs& a, const ConvShape& s) {
    const ConvLayer* L = a.layer;
    return 2.0 * (double)a.x0.B * s.Wout * s.Hout * L->Cout * ((double)L->Cin * s.taps + (L->sc_identity ? 0.0 : (double)L->R));
}
static double conv_bytes(const ConvArgs& a, const ConvShape& s, size_t out_copies = 1, bool res_weights = true) {
    const ConvLayer* L = a.layer;
    const double out_px = (double)a.x0.B * s.Wout * s.Hout;
    return (double)a.x0.B * a.x0.W * a.x0.H * s.Cin_t * 2.0 + (double)L->Cout * (L->Cin * s.taps + (res_weights ? L->R : 0)) * 2.0 +
           out_px * L->Cout * (a.out_f32_nchw ? 4.0 : 2.0) * (double)out_copies + out_px * s.R_t * 2.0;
}

// what a conv launch takes from the plan's I/O block every time it runs (the block's owner may rebind it between runs); an
// emitter names the members its kernel reads
struct ConvLate {
    int temb_off = -1;             // >= 0: the time-embedding table at this channel offset, and the step index that selects its row
    bool first_of_step = false;    // advances the sampler's step index when the pack_input launch is fused away
    bool f32_out = false;          // writes io.out
    bool sch = false;              // ... through the scheduler step
    void apply(ConvParams& p, const PlanIO& io) const {
        if (first_of_step) p.step_inc = io.pack_fused ? io.step_inc : nullptr;
        if (temb_off >= 0) {
            p.temb = io.temb + temb_off;
            p.step_ptr = io.step_ptr;
            p.temb_rows_per_step = io.temb_rows_per_step;
            p.temb_per_sample = io.temb_per_sample;
        }
        if (f32_out) p.y_nchw = io.out;
        if (sch) p.sch = io.sch;
    }
};

void ViewPlan::decide() {
    std::map<int, int> nper;
    for (auto& kv : cons) {
        Cons& c = kv.second;
        bool good = c.ok && c.groups > 0 && c.Ctot % c.groups == 0;
        const int cpg = good ? c.Ctot / c.groups : 0;
        good = good && cpg >= 1 && cpg <= 32 && (cpg & (cpg - 1)) == 0;
        for (auto& pt : c.parts)
            good = good && pt.prod >= 0 && pt.prod < (int)can_emit.size() && can_emit[pt.prod] && pt.ch_off % cpg == 0 &&
                   nper[pt.prod] < 3;
        c.use = good;
        if (!good) continue;
        for (auto& pt : c.parts) {
            emit[pt.prod].push_back({kv.first, pt.ch_off, c.Ctot, c.silu, c.groups, c.eps});
            nper[pt.prod]++;
        }
    }
}

int Plan::run(hipStream_t s) {
    for (auto& o : ops)
        if ((!o.active || o.active()) && o.fn(s)) return 1;
    return 0;
}
// same, with a timestamp launch around every op (rldm_debug_graph_trace: the timeline of the ops as they run
// back to back inside the captured graph, which a host-side profiler cannot see without spacing them out)
int Plan::run_stamped(hipStream_t s, unsigned long long* slots, int cap) {
    if (launch_stamp(slots, s)) return 1;
    int n = 0;                              // (ops that launch nothing this run leave no stamp)
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].active && !ops[i].active()) continue;
        if (ops[i].fn(s)) return 1;
        ++n;
        if (n < cap && launch_stamp(slots + n, s)) return 1;
    }
    return 0;
}
// eager pass with a HIP event pair around every launch on `s` (the stream the kernels run on)
int Plan::run_profiled(hipStream_t s, std::map<std::string, KernelStat>& stats) {
    std::vector<hipEvent_t> ev(ops.size() + 1);
    for (auto& e : ev) RLDM_HIP_CHECK(hipEventCreate(&e));
    RLDM_HIP_CHECK(hipEventRecord(ev[0], s));
    std::vector<char> ran(ops.size(), 1);
    for (size_t i = 0; i < ops.size(); ++i) {
        ran[i] = !ops[i].active || ops[i].active();
        if (ran[i] && ops[i].fn(s)) return 1;
        RLDM_HIP_CHECK(hipEventRecord(ev[i + 1], s));
    }
    RLDM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < ops.size(); ++i) {
        if (!ran[i]) continue;
        float ms = 0.f;
        RLDM_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        KernelStat& k = stats[ops[i].name];
        k.launches += 1;
        k.ms += ms;
        k.flops += ops[i].flops;
        k.bytes += ops[i].bytes;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return 0;
}

struct TileChoice {
    ConvTile tile;
    int TW = 1, TH = 1, ksplit = 1;
};

// output-pixel tile of a block: as tall as the image allows (<= 16 beams), then as wide as BM allows
static void pixel_tile(int BM, int Wout, int Hout, int* TW, int* TH) {
    int th = 1;
    while (th * 2 <= Hout && th * 2 <= 16 && Hout % (th * 2) == 0) th *= 2;
    int tw = 1;
    while (tw * 2 * th <= BM && Wout % (tw * 2) == 0) tw *= 2;
    *TW = tw;
    *TH = th;
}

static TileChoice choose_tile(long long B, int Wout, int Hout, int stride, int N, int Cin_pad, int C0, int R, int R0,
                              int taps, bool nchw, bool gn) {
    TileChoice c;
    const int KW = taps == 9 ? 3 : 1;
    // a channel chunk never straddles a concat boundary
    auto ck_ok = [&](int ck) { return Cin_pad % ck == 0 && C0 % ck == 0 && R % ck == 0 && R0 % ck == 0; };
    // instance for a (BM, BN): the widest channel chunk it exists with
    auto pick = [&](int BM, int BN, ConvTile* u, int* tw, int* th) {
        const int cks[3] = {64, 32, 16};
        for (int ck : cks) {
            if (!ck_ok(ck)) continue;
            ConvTile v;
            v.BM = BM; v.BN = BN; v.CK = ck; v.taps = taps;
            if (!conv_tile_supported(v)) continue;
            pixel_tile(BM, Wout, Hout, tw, th);
            // shrink the tile until the halo fits the instance's register staging capacity
            bool ok = true;
            while (((*tw - 1) * stride + KW) * ((*th - 1) * stride + KW) > conv_max_halo_slots(v)) {
                if (*tw > 1) *tw >>= 1; else if (*th > 1) *th >>= 1; else { ok = false; break; }
            }
            if (!ok) continue;
            *u = v;
            return true;
        }
        return false;
    };
    auto blocks = [&](const ConvTile& u, int tw, int th) {
        return B * (Wout / tw) * (Hout / th) * ((N + u.BN - 1) / u.BN);
    };
    const int bn_pref = N <= 32 ? 32 : (N <= 64 ? 64 : 128);
    // candidates in order of preference (preferred channel tile first, largest pixel tile first); take the first that
    // fills the chip, else the one with the most blocks.  Pass 1 also accepts tiles that are mostly padding; pass 2 any
    // channel tile (small test configurations have few instances).
    const int bms[3] = {256, 128, 64};
    std::vector<int> bns = {bn_pref};
    if (bn_pref > 64) bns.push_back(64);
    long long best_blocks = -1;
    TileChoice best;
    bool found = false;
    for (int pass = 0; pass < 3 && best_blocks < 0; ++pass) {
        if (pass == 2) bns = {32, 64, 128};
        for (int bi = 0; bi < 3 && !found; ++bi)
            for (size_t ni = 0; ni < bns.size() && !found; ++ni) {
                ConvTile u;
                int tw, th;
                if (!pick(bms[bi], bns[ni], &u, &tw, &th)) continue;
                // more than half empty: try a smaller BM first -- except under stride 2, where the halo capacity shrinks the
                // pixel tile of every instance and the 256-pixel one-tap pipeline still wins when it fills the chip (measured)
                if (pass == 0 && tw * th * 2 <= u.BM && bi < 2 && !(stride == 2 && bi == 0)) continue;
                const long long nb = blocks(u, tw, th);
                if (nb > best_blocks) {
                    best_blocks = nb;
                    best.tile = u;
                    best.TW = tw;
                    best.TH = th;
                }
                // enough blocks?  A 1x1 conv with a GroupNorm prologue (attention q/k/v) re-normalises its input once per
                // channel tile, so a wide tile on half the CUs beats two rounds of narrow ones (measured, tools/bench_conv.py)
                if (nb >= ((taps == 1 && gn) ? 128 : 200)) found = true;
            }
    }
    if (g_force_bm && g_force_bn) {
        ConvTile u;
        int tw, th;
        if (pick(g_force_bm, g_force_bn, &u, &tw, &th)) {
            best.tile = u;
            best.TW = tw;
            best.TH = th;
            best_blocks = blocks(u, tw, th);
        }
    }
    c = best;
    if (best_blocks < 0) {
        c.tile.BM = 64; c.tile.BN = 64; c.tile.CK = 16; c.tile.taps = taps;
        return c;                    // caller reports "no kernel instance" if this one does not exist either
    }
    // split-K over channel chunks only on request (rldm_debug_force_tile): the in-launch combine costs more than the idle CUs
    // (DESIGN.md); fp32 NCHW outputs never split
    c.ksplit = 1;
    const int ncc = Cin_pad / c.tile.CK;
    if (!nchw && g_force_ks > 0 && g_force_ks <= std::max(1, ncc)) c.ksplit = g_force_ks;
    return c;
}

// recording pass: GroupNorm `n` over cat[x0, x1] is consumed by something that could read a pre-activated tensor instead
void Builder::record_consumer(const NormParams* n, const Tensor& x0, const Tensor& x1, int silu, bool ok, int groups, float eps) {
    if (!vp || !recording || !n) return;
    ViewPlan::Cons c;
    c.parts.push_back({x0.prod, 0});
    if (x1.valid()) c.parts.push_back({x1.prod, x0.C});
    c.Ctot = x0.C + (x1.valid() ? x1.C : 0);
    c.silu = silu;
    c.groups = groups;
    c.eps = eps;
    c.ok = ok && x0.W * x0.H == (x1.valid() ? x1.W * x1.H : x0.W * x0.H);
    vp->cons[n] = c;
}
// sizing / real pass: the pre-activated input of the consumer that owns norm `n`, if the plan has one
bool Builder::take_view(const NormParams* n, Tensor* v) {
    if (!vp || recording || !n) return false;
    auto it = vp->cons.find(n);
    if (it == vp->cons.end() || !it->second.use) return false;
    auto vt = view_tensors.find(n);
    if (vt == view_tensors.end()) return false;
    *v = vt->second;
    view_tensors.erase(vt);
    return true;
}

Tensor Builder::make(int B, int W, int H, int C) {
    Tensor t;
    t.B = B; t.W = W; t.H = H; t.C = C;
    t.id = next_id++;
    t.off = arena.alloc(t.bytes());
    refs[t.id] = 1;
    live[t.id] = t;
    return t;
}
void Builder::add_stats(Tensor& t, int P) {
    t.P = P;
    t.st_off = arena.alloc(t.st_bytes());
    live[t.id] = t;
}
void Builder::release(const Tensor& t) {
    if (!t.valid()) return;
    if (trunk_open) {          // (the memory may not be recycled inside the segment)
        deferred.push_back(t);
        return;
    }
    if (--refs[t.id] == 0) {
        arena.release(t.off, t.bytes());
        if (t.P) arena.release(t.st_off, t.st_bytes());
        live.erase(t.id);
    }
}
int Builder::flush_trunk() {
    if (!trunk_open) return 0;
    trunk_open = false;
    int rc = 0;
    // the runtime's own answer to "are all these workgroups resident at once?" (variant 4: two per CU) -- asked here, at plan build,
    // not left to the launch's bounded-wait self-check.  A query that FAILS (< 0) changes nothing; a clear "no" keeps the layers launches.
    const int need_per_cu = pend.variant == 4 ? 2 : 1;
    const int resident = (!dry && pend.phases.size() > 1) ? trunk_max_resident(pend.variant, pend.lds) : need_per_cu;
    const bool not_resident = resident >= 0 && resident < need_per_cu && pend.standalone.size() == pend.phases.size();
    if (not_resident) {
        static bool said = false;
        if (!said) fprintf(stderr, "librangeldm_hip: trunk_kernel<%d> with %zu bytes of LDS: %d workgroup(s) per CU resident, %d needed; "
                           "these layers run as launches of their own\n", pend.variant, pend.lds, resident, need_per_cu);
        said = true;
        launches += (int)pend.standalone.size() - 1;
        for (auto& op : pend.standalone) plan->ops.push_back(op);
    } else if (!dry && pend.phases.size() == 1 && pend.standalone.size() == 1) {
        plan->ops.push_back(pend.standalone[0]);
    } else if (!dry && !pend.phases.empty()) {
        auto recs = std::make_unique<DevBuf>();
        auto ctrs = std::make_unique<DevBuf>();
        if (upload(*recs, pend.phases.data(), pend.phases.size() * sizeof(TrunkPhase))) return 1;
        if (ctrs->alloc((size_t)pend.B * 32 * 4)) return 1;
        RLDM_HIP_CHECK(hipMemset(ctrs->p, 0, ctrs->bytes));
        if (!plan->trunk_error.p) {
            if (plan->trunk_error.alloc(64)) return 1;
            RLDM_HIP_CHECK(hipMemset(plan->trunk_error.p, 0, 64));
        }
        TrunkParams tp;
        memset(&tp, 0, sizeof(tp));
        tp.phases = recs->as<TrunkPhase>();
        tp.nphases = (int)pend.phases.size();
        tp.B = pend.B;
        tp.ranks = pend.ranks;
        tp.ntile_n = pend.nwn == 1 ? pend.ranks : pend.ntile_n;
        tp.nwn = pend.nwn;
        tp.variant = pend.variant;
        tp.skew = 0;                    // (variant 4 can start its second image group late: no offset measured faster, docs/history/rounds1-4.md)
        tp.counters = ctrs->as<unsigned>();
        tp.error = plan->trunk_error.as<int>();
        tp.temb_ld = temb_ld;
        plan->trunk_bufs.push_back(std::move(recs));
        plan->trunk_bufs.push_back(std::move(ctrs));
        Plan* pl = plan;
        const size_t lds = pend.lds;
        const bool ts_ok = !stamp_env().trunk_first || ++trunk_seen[(int)pend.phases.size()] == 1;   // (timeline of the FIRST such launch)
        plan->ops.push_back({[tp, lds, pl, ts_ok](hipStream_t st) mutable {
            tp.temb = pl->io.temb;
            tp.step_ptr = pl->io.step_ptr;
            tp.temb_rows_per_step = pl->io.temb_rows_per_step;
            tp.temb_per_sample = pl->io.temb_per_sample;
            tp.ts = ts_ok ? stamp_buf(StampSite::Trunk, tp.nphases) : nullptr;
            return launch_trunk(tp, lds, st);
        }, std::string("trunk_kernel<") + (pend.variant == 0 ? "conv_small image tiles" : pend.variant == 1 ? "conv_small 64x64 clusters" :
                                           pend.variant == 2 ? "conv_stream 256x128" : "conv_stream 128x128 x2/CU") +
               ", " + std::to_string(pend.phases.size()) + " phases>", pend.flops, pend.bytes});
    }
    pend = PendingTrunk();
    std::vector<Tensor> d;
    d.swap(deferred);
    for (const Tensor& t : d) release(t);
    return rc;
}

bool Builder::trunk_attention_ok(const Tensor& x, bool pre) const {
    const int L = x.W * x.H, ranks = x.C / own_tile_channels(x.B, L, x.C);
    // (x.C % 64: attention_qkv2_body loads x in coalesced 64-channel groups and projects in blocks of 4 k-steps, no tail)
    if (!trunk_enabled() || !pre || x.C % 64 != 0 || ranks < 2 || ranks > 16) return false;
    const int HG = (x.C / 8) / ranks, wph = (L + 31) / 32;
    // 8 waves: one query tile per wave of a head (32-token images -- the lowest nuScenes level -- leave every second wave idle:
    // without the phase that level was five persistent launches with an attention launch between each pair)
    if (HG * wph > 8 || 8 % HG != 0 || (8 / HG) < wph || L > 64) return false;
    if (!trunk_grid_fits(ranks, x.B)) return false;
    return trunk_attention_lds(L, x.C, HG) <= 160 * 1024;
}
// ... of a multi-tile cluster: raw x + statistics (the fold runs inside the phase), two query tiles per wave; 0: not eligible
int Builder::cluster_attention_ranks(const Tensor& x, bool pre) const {
    const int L = x.W * x.H, ranks = cluster_ranks(x.B, x.C, L);
    if (!cluster_enabled() || pre || ranks == 0 || x.P <= 0 || (x.C / 8) % ranks != 0 || L % 32 != 0) return 0;
    const int HG = (x.C / 8) / ranks, wph = L / 32;
    if (HG * wph != 16 || x.C > 512) return 0;                // 8 waves x two query tiles
    return trunk_attention_lds(L, x.C, HG) <= 160 * 1024 ? ranks : 0;
}
int Builder::device_cus() {
    static int cus = [] { int dev = 0, n = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0; return n; }();
    return std::min(256, cus > 0 ? cus : 256);
}
// (round 5) channels per image-owning tile: 16 for the 64-pixel images of the KITTI network's 32x2 level (256 output channels -> 16
// workgroups per image), when that grid is resident at once; 32 otherwise.  (Also without persistent launches: the per-layer
// fall-back keeps their tiles, so its results stay identical.)
int Builder::own_tile_channels(int B, int npix, int N) const {
    return (npix == 64 && N == 256 && trunk_grid_fits(16, B)) ? 16 : 32;
}
void Builder::trunk_begin(int B, int ranks, int ntile_n, int nwn, int variant) {
    if (nwn == 1) ntile_n = ranks;
    if (variant < 0) variant = nwn == 1 ? 0 : 1;
    if (trunk_open && (pend.ranks != ranks || pend.B != B || pend.nwn != nwn || pend.ntile_n != ntile_n || pend.variant != variant))
        flush_trunk();
    if (!trunk_open) {
        ++launches;
        trunk_open = true;
        pend.B = B;
        pend.ranks = ranks;
        pend.ntile_n = ntile_n;
        pend.nwn = nwn;
        pend.variant = variant;
    }
}
int Builder::cluster_ranks(int B, int C, int npix) const {
    if (C % 64 != 0 || npix % 64 != 0) return 0;
    const int r = (C / 64) * (npix / 64);
    return (r >= 2 && r <= 16 && npix > 64 && trunk_grid_fits(r, B)) ? r : 0;
}
void Builder::trunk_push_attention(const AttnQkvParams& ap, double fl, double by) {
    TrunkPhase ph = trunk_attention_phase(ap);
    ph.w[TW_WBYTES] = (unsigned)(3 * ap.C * ap.C * 2);          // q / k / v projection fragments (attention_body.h)
    pend.phases.push_back(ph);
    pend.lds = std::max(pend.lds, trunk_attention_lds(ap.L, ap.C, (ap.C / 8) / pend.ranks));
    pend.flops += fl;
    pend.bytes += by;
}

// per-channel statistics of a tensor that did not come out of a conv epilogue (external inputs in the test entry points)
int Builder::gn_stats(Tensor& x) {
    const int npix = x.W * x.H;
    const int P = std::max(1, std::min(16, npix / 64));
    add_stats(x, P);
    note_launch();
    if (!dry) {
        GnStatsParams g;
        g.x = tptr(x);
        g.C = x.C;
        g.B = x.B;
        g.npix = npix;
        g.P = P;
        g.part = ptr<float2>(x.st_off);
        const double by = (double)x.B * npix * x.C * 2.0;
        plan->ops.push_back({[g](hipStream_t s) { return launch_gn_stats(g, s); }, "gn_stats_kernel", 0.0, by});
    }
    return 0;
}

// ---- convs: conv_route asks each route's *_params in turn; the first that admits the conv has filled its ConvParams, and the
// route's emitter (conv_small, conv_stream, ...) takes them from there.  What every route does the same way is stated once here.

// the fields all routes fill alike: channels, sizes, the pixel tile (s.Wout x s.Hout cut into TW x TH) and the reciprocals
// the kernels divide with; thv: halo rows of a tile (0: the route's kernels do not divide by it)
void Builder::conv_geometry(const ConvArgs& a, const ConvShape& s, int TW, int TH, int thv, ConvParams* q) {
    memset(q, 0, sizeof(*q));
    q->C0 = a.x0.C;
    q->C1 = s.Cin_t - a.x0.C;
    q->R0 = a.r0.valid() ? a.r0.C : 0;
    q->R1 = s.R_t - q->R0;
    q->B = a.x0.B; q->Win = a.x0.W; q->Hin = a.x0.H;
    q->up = a.up; q->stride = a.stride;
    q->pad_lo = (s.taps == 1) ? 0 : (a.pad_mode == 0 ? 1 : 0);
    q->Wout = s.Wout; q->Hout = s.Hout;
    q->TW = TW; q->TH = TH;
    while ((1 << q->th_shift) < TH) ++q->th_shift;
    q->tiles_h = s.Hout / TH;
    q->tiles_img = (s.Wout / TW) * q->tiles_h;
    if (thv) q->magic_thv = ((1 << 20) + thv - 1) / thv;
    const int cpg = std::max(1, s.Cin_t / a.groups);
    q->magic_cpg = ((1 << 20) + cpg - 1) / cpg;
    q->gn_inv_n = (float)(1.0 / ((double)a.x0.W * a.x0.H * cpg));
    q->N = a.layer->Cout;
    q->silu = a.silu;
    q->gn_eps = a.eps;
    q->gn_groups = a.groups;
    q->ksplit = 1;
}
int Builder::require_gn_input(const ConvArgs& a, int Cin_t) const {
    if (!a.gn) return 0;
    RLDM_REQUIRE(a.gn->C == Cin_t && Cin_t % a.groups == 0, "conv " + a.layer->name + ": GroupNorm channel mismatch");
    RLDM_REQUIRE(a.x0.P > 0 && (!a.x1.valid() || a.x1.P > 0), "conv " + a.layer->name + ": GroupNorm input without statistics");
    return 0;
}
// real pass: the device pointers of a conv launch -- inputs, residual sources, weights, the GroupNorm prologue's statistics
// and affine, the bf16 output y (invalid: the layer writes plan->io.out, bound when the launch runs)
void Builder::bind_conv(ConvParams& p, const ConvArgs& a, const ConvLayer::Packed& pk, const Tensor& y) const {
    p.x0 = tptr(a.x0);
    p.x1 = tptr(a.x1);
    p.r0 = tptr(a.r0);
    p.r1 = tptr(a.r1);
    p.wpk = pk.w.as<bf16_t>();
    p.bias = pk.bias.as<float>();
    if (a.gn) {
        p.st0 = sptr(a.x0);
        p.st1 = sptr(a.x1);
        p.P0 = a.x0.P;
        p.P1 = a.x1.valid() ? a.x1.P : 0;
        p.gn_gamma = a.gn->gamma.as<float>();
        p.gn_beta = a.gn->beta.as<float>();
    }
    if (y.valid()) {
        p.y = tptr(y);
        p.y_ld = y.C;
        p.y_stats = y.P ? ptr<float2>(y.st_off) : nullptr;
    }
    p.temb_ld = temb_ld;
}

// conv_small.hip route: 3x3 / stride 1 convs over <= 256-pixel images (the 64x4 and 32x2 UNet levels) and every
// pointwise conv with 128..512 input channels (attention q/k/v and output projections)
void Builder::small_tile(int bm, int Wout, int Hout, int* tw, int* th) {
    int h = 1;
    while (h * 2 <= Hout && h * 2 <= 8 && Hout % (h * 2) == 0) h *= 2;
    *th = h;
    *tw = bm / h;
}
// geometry + channel counts of the route; `epi_res`: the identity residual is added in the epilogue instead of the K loop
bool Builder::small_params(const ConvArgs& a, const ConvShape& s, ConvParams* q, bool* epi_res) {
    const int Cin_t = s.Cin_t, R_t = s.R_t, taps = s.taps, Wout = s.Wout, Hout = s.Hout;
    if (dbg() & RLDM_FLAG_NO_CONV_SMALL) return false;
    if ((taps != 9 && taps != 1) || a.stride != 1 || (a.up != 1 && !(a.up == 2 && taps == 9 && !a.gn && R_t == 0)) || a.out_f32_nchw)
        return false;
    // (128-pixel tiles for the 128x8 level are built and tested but lose to the generic kernel there: the separate
    //  GroupNorm pass over a 12 MB tensor costs more than the faster K loop wins; RLDM_FLAG_SMALL_128PX routes them)
    // small images (C2: the 64x4 / 32x2 levels at batch 16), or few pixels in the whole batch (C1 / C3: 128x8 at batch 1,
    // 128x4 at batch 4): the same 64-pixel tiles, more of them per image
    const bool few_px = (long long)a.x0.B * Wout * Hout <= 4096;
    if (taps == 9 && (a.pad_mode != 0 || (Wout * Hout > ((dbg() & RLDM_FLAG_SMALL_128PX) ? 1024 : 256) && !few_px))) return false;
    // pixel tile: 64; 128 for the 3x3 convs of the 128x8 level (each weight fragment then feeds 4 MFMAs)
    // (32 for 32x1 images: the lowest nuScenes level, which otherwise runs as 8 workgroups of the generic kernel; and for
    //  32x2 images, as two tiles each: twice the workgroups, half the staging / epilogue per workgroup -- level-3 convs
    //  13.4-14.2 -> 13.0 us, +0.5-1 % end to end; RLDM_FLAG_SMALL_64PX_32X2 keeps the 64-pixel tile: tests)
    int bm = (taps == 9 && Wout * Hout > 256 && !few_px) ? 128 :
             ((Wout * Hout == 32 || (Wout * Hout == 64 && Hout == 2 && !(dbg() & RLDM_FLAG_SMALL_64PX_32X2))) && a.up == 1 ? 32 : 64);
    if (a.own_image) {                      // one tile per image (<= 64 pixels), or not this route
        if (Wout * Hout > 64 || a.up != 1) return false;
        bm = Wout * Hout;
    }
    if (taps == 1 && a.x1.valid()) return false;
    if (!a.gn && a.x1.valid()) return false;
    if (a.layer->Cout % 32 != 0 || (g_force_bm && g_force_bm != 64)) return false;
    int tw, th;
    small_tile(bm, Wout, Hout, &tw, &th);
    if (Wout % tw != 0 || Hout % th != 0 || Wout < 2) return false;
    *epi_res = a.layer->sc_identity && a.r0.valid() && !a.r1.valid() && a.r0.C == a.layer->Cout;
    conv_geometry(a, s, tw, th, 0, q);
    if (!(taps == 9 && a.x1.valid() && small_gn_fused(a, taps))) {     // (that: a concatenated input normalised by the conv's own staging)
        q->C0 = Cin_t;                      // one input tensor: single, or pre-activated by gn_apply
        q->C1 = 0;
    }
    if (*epi_res) q->R0 = q->R1 = 0;
    q->colb = conv_small_col_bytes(Cin_t, th, taps);
    return true;
}
// channel tile; 0: no instance / not worth it.
// 3x3: 64 channels when that fills the chip, else 32 (twice the blocks, half the weight stream per block).
// 1x1: the work per block is a few MFMAs and the launch is one latency chain per block, so the route is taken only if
// the grid fits one round of 256 workgroups -- with the narrowest tile that does (most blocks); else the generic kernel.
int Builder::small_bn(const ConvParams& q, int taps, bool gn_fused, bool own) {
    const auto supported = [&](int bn) {
        return supported_with(q, gn_fused, false, [&](const ConvParams& t) { return conv_small_supported(t, taps, bn); });
    };
    const long long tiles = (long long)q.B * q.tiles_img;
    if (own) return (q.tiles_img == 1 && supported(32)) ? 32 : 0;      // whole groups per 32-channel tile
    if (g_force_bn && supported(g_force_bn)) return g_force_bn;
    if (taps == 9 && q.TW * q.TH == 128)    // one round of workgroups, or the generic kernel
        return (supported(64) && tiles * (q.N / 64) <= 256) ? 64 : 0;
    if (taps == 9) {
        const bool ok64 = supported(64), ok32 = supported(32);
        if (ok64 && (tiles * (q.N / 64) >= 200 || !ok32)) return 64;
        // (measured, round 3: giving a level that COULD run as multi-tile clusters the cluster's 64 x 64 tile at small batches --
        //  nuScenes 64x2 at 4 images: 66 -> 42 launches per step -- is slower, 84.3 against 86.9 img/s, and neutral for the KITTI
        //  network at 4 / 8 images: a phase costs what a launch costs; the 32-channel tiles' extra workgroups win)
        return ok32 ? 32 : 0;
    }
    const int cand[3] = {32, 64, 128};
    for (int bn : cand)
        if (supported(bn) && tiles * (q.N / bn) <= 256) return bn;
    return 0;
}
// GroupNorm (+ SiLU) folded into the conv's staging: every 1x1, and the 3x3 convs over ONE input tensor (a concatenated
// input on an image-owning tile keeps the separate gn_apply launch / phase)
// (round 4) ... and a concatenated 3x3 input on tiles that do not own their image (the 64x4 level's cluster phases, the stand-alone
// launches of the small-batch configurations): the gn_apply phase / launch it replaces costs 12-23 k cycles, the four-fold repeated
// arithmetic in the staging ~4.7 k
bool Builder::small_gn_fused(const ConvArgs& a, int taps) {
    if (a.gn == nullptr) return false;
    if (taps == 1) return true;
    return !a.x1.valid() || (!a.own_image && a.x0.C % 8 == 0 && a.x1.C % 8 == 0);
}
// does the route take this conv?  If so *q, *epi_res and *bn (the channel tile) are what conv_small runs it with
bool Builder::small_route(const ConvArgs& a, const ConvShape& s, ConvParams* q, bool* epi_res, int* bn) {
    if (!small_params(a, s, q, epi_res)) return false;
    *bn = small_bn(*q, s.taps, small_gn_fused(a, s.taps), a.own_image);
    return *bn != 0;
}
// ... asked about a conv that is not being built (the recording pass, the wide-concat resnet's choice of layers)
bool Builder::small_route(const ConvArgs& a, const ConvShape& s) {
    ConvParams q;
    bool epi;
    int bn;
    return small_route(a, s, &q, &epi, &bn);
}

// p, epi_res, BN: as small_route decided them
int Builder::conv_small(const ConvArgs& a, const ConvShape& s, ConvParams p, bool epi_res, int BN, Tensor* out) {
    ConvLayer* L = a.layer;
    const int N = L->Cout, Cin_t = s.Cin_t, taps = s.taps, Wout = s.Wout, Hout = s.Hout;
    const bool gn_fused = small_gn_fused(a, taps);         // folded into the conv's staging
    const bool preact = a.gn != nullptr && !gn_fused;      // concatenated 3x3 input: GroupNorm + SiLU in their own launch
    if (require_gn_input(a, Cin_t)) return 1;
    Tensor act;
    if (preact) act = make(a.x0.B, a.x0.W, a.x0.H, Cin_t);
    const Tensor& x0 = preact ? act : a.x0;
    p.dbg = kernel_dbg();
    p.ts = stamp_buf(StampSite::Conv, conv_ord - 1);
    // (round 5) image-owning tiles of the 32x2 level: 16 channels per workgroup -- the level's persistent launch then runs on 16
    // workgroups per image (all 256 CUs at batch 16) with half the K loop, weight stream and epilogue per workgroup
    if (BN == 32 && a.own_image && own_tile_channels(x0.B, p.TW * p.TH, N) == 16 && !gn_fused && conv_small_supported(p, taps, 16)) BN = 16;
    p.ntile_n = N / BN;

    Tensor y = make(x0.B, Wout, Hout, N);
    if (a.want_stats || a.own_image) add_stats(y, p.tiles_img);
    // normalised copies for the consumers (producer-side GroupNorm): the consumer's input tensor is created by the first
    // producer that writes a part of it and released by the consumer
    std::vector<Tensor> vts;
    if (a.own_image && cur_emit) {
        RLDM_REQUIRE(p.tiles_img == 1 && cur_emit->size() <= 3, "conv " + L->name + ": producer-side GroupNorm lost its tile");
        for (const auto& e : *cur_emit) {
            auto it = view_tensors.find(e.norm);
            if (it == view_tensors.end()) it = view_tensors.emplace(e.norm, make(x0.B, Wout, Hout, e.Ctot)).first;
            vts.push_back(it->second);
        }
    }
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    // a phase of the persistent trunk launch (trunk.hip) instead of a launch of its own: the tile owns the image, the input
    // arrives pre-activated (or needs no norm), one of the three instances the trunk kernel carries
    const int px_t = p.TW * p.TH;
    const int kind_l = (taps == 9 && Cin_t == 256) ? 0 : ((taps == 9 && Cin_t == 512) ? 1 : ((taps == 1 && Cin_t == 256) ? 2 : -1));
    const int trunk_kind = kind_l < 0 ? -1 : kind_l + (BN == 16 ? TK_H16 : (px_t == 32 ? 4 : 0));      // (+4: the 32-pixel instances; +16: 16-channel tiles)
    const int ranks_t = N / BN;
    bool in_trunk = trunk_enabled() && a.own_image && p.tiles_img == 1 && (BN == 32 || BN == 16) && (px_t == 64 || px_t == 32) && !gn_fused &&
                    trunk_kind >= 0 && p.up == 1 && ranks_t >= 2 && ranks_t <= 16 && trunk_grid_fits(ranks_t, x0.B) &&
                    2 * p.TH * (Cin_t / 8) <= 512 && vts.size() <= 2;
    // (a concatenated input is normalised by a gn_apply phase in front of the conv's -- or the conv stays a launch of its own)
    const bool gn_phase_t = in_trunk && preact && Cin_t <= 512 && (Wout * Hout) % ranks_t == 0 && a.x0.C % 8 == 0 &&
                            (!a.x1.valid() || a.x1.C % 8 == 0);
    in_trunk = in_trunk && (!preact || gn_phase_t);
    // ... or a phase of a MULTI-TILE cluster (the 64x4 level at batch <= 16): conv_small's default 64-pixel x 64-channel tiles, the
    // consumer-side GroupNorm fold stays inside the phase
    // (3x3 over 128 channels -- the all-taps-ring instance, 211 registers on its own -- does not fit beside the phase loop's state)
    const int kind_c = (taps == 9 && Cin_t == 128) ? TK_CL_3x3_128 : (taps == 9 && Cin_t == 256) ? TK_CL_3x3_256 :
                       (taps == 9 && Cin_t == 384) ? TK_CL_3x3_384 : (taps == 9 && Cin_t == 512) ? TK_CL_3x3_512 :
                       (taps == 1 && Cin_t == 256) ? TK_CL_1x1_256 : -1;
    const int ranks_c = cluster_ranks(x0.B, N, Wout * Hout);
    const bool in_cluster = !in_trunk && cluster_enabled() && !a.own_image && kind_c >= 0 && BN == 64 && px_t == 64 &&
                            (p.up == 1 || p.up == 2) && vts.empty() && ranks_c == (N / 64) * p.tiles_img &&
                            p.Win * p.up == Wout && p.Hin * p.up == Hout;
    // GroupNorm + SiLU once, ahead of the conv: every channel tile of the conv would otherwise redo it (4-8x at these levels) --
    // as a launch (norm.hip) or, in front of a multi-tile cluster phase, as a phase of the same persistent launch
    if (preact) {
        const bool gn_phase = gn_phase_t || (in_cluster && Cin_t <= 512 && (Wout * Hout) % ranks_c == 0 && a.x0.C % 8 == 0 &&
                                             (!a.x1.valid() || a.x1.C % 8 == 0));
        if (gn_phase_t) trunk_begin(x0.B, ranks_t);
        else if (gn_phase) trunk_begin(x0.B, ranks_c, N / 64, 2);
        else note_launch();
        if (!dry) {
            GnApplyParams g;
            memset(&g, 0, sizeof(g));
            g.x0 = tptr(a.x0); g.x1 = tptr(a.x1);
            g.C0 = a.x0.C; g.C1 = a.x1.valid() ? a.x1.C : 0;
            g.st0 = sptr(a.x0); g.st1 = sptr(a.x1);
            g.P0 = a.x0.P; g.P1 = a.x1.valid() ? a.x1.P : 0;
            g.B = a.x0.B; g.npix = a.x0.W * a.x0.H;
            g.groups = a.groups;
            g.gamma = a.gn->gamma.as<float>(); g.beta = a.gn->beta.as<float>();
            g.eps = a.eps; g.silu = a.silu;
            g.y = tptr(act);
            const double by = (double)g.B * g.npix * Cin_t * 4.0;
            if (gn_phase) {
                g.inv_n = (float)(1.0 / ((double)g.npix * (Cin_t / g.groups)));      // (what launch_gn_apply sets for the launch)
                pend.phases.push_back(trunk_gn_apply_phase(g));
                pend.lds = std::max(pend.lds, (size_t)(2 * 512 * 8 + 2 * 512 * 4));
                pend.bytes += by;
            }
            emit({[g](hipStream_t st) { return launch_gn_apply(g, st); }, "gn_apply_kernel", 0.0, by}, gn_phase);
        }
    }
    if (in_trunk) trunk_begin(x0.B, ranks_t);
    else if (in_cluster) trunk_begin(x0.B, ranks_c, N / 64, 2);
    else note_launch();
    in_trunk = in_trunk || in_cluster;
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (L->get_fragpacked(Cin_t, BN == 16 ? 16 : 32, BN == 16 ? 8 : conv_small_kgroups(BN), epi_res, &pk)) return 1;
        ConvArgs k = a;                     // what the kernel itself reads:
        k.x0 = x0;                          // the pre-activated copy;
        if (!gn_fused) k.gn = nullptr;      // a GroupNorm only when it is folded into the staging,
        if (!gn_fused || p.C1 == 0) k.x1 = Tensor();                   // ... the second tensor of a concat only under it;
        if (epi_res) {                      // the identity residual in the epilogue, not as a K phase
            p.res = tptr(a.r0);
            k.r0 = k.r1 = Tensor();
        }
        bind_conv(p, k, *pk, y);
        for (size_t v = 0; v < vts.size(); ++v) {
            const auto& e = (*cur_emit)[v];
            NormView& nv = p.nv[v];
            nv.y = tptr(vts[v]) + e.ch_off;
            nv.gamma = e.norm->gamma.as<float>() + e.ch_off;
            nv.beta = e.norm->beta.as<float>() + e.ch_off;
            nv.ld = e.Ctot;
            const int cpg = e.Ctot / e.groups;
            nv.cpg_shift = 0;
            while ((1 << nv.cpg_shift) < cpg) ++nv.cpg_shift;
            nv.inv_n = (float)(1.0 / ((double)Wout * Hout * cpg));
            nv.eps = e.eps;
            nv.silu = e.silu;
        }
        p.nviews = (int)vts.size();
        Plan* pl = plan;
        const int temb_off = a.temb_off;
        const double by = conv_bytes(a, s, 1 + vts.size());
        const std::string kname = "conv_small_kernel<" + std::to_string(p.TW * p.TH) + "," + std::to_string(BN) + ",taps" + std::to_string(taps) + ">";
        if (in_trunk) {
            RLDM_REQUIRE(!in_cluster || p.nviews == 0, "conv " + L->name + ": a multi-tile cluster phase writes no views");
            TrunkPhase ph = trunk_conv_phase(p, in_cluster ? kind_c : trunk_kind, in_cluster, temb_off);
            // the wave's weight stream: k-groups, channels per k-step, k-steps per tap and k-group; fragments in its ring (conv_small_body.h)
            const int KG = in_cluster ? 4 : 8, ksc = BN == 16 ? 32 : 16, cpt = Cin_t / (ksc * KG);
            int G;
            if (in_cluster) G = (taps == 1 ? 1 : (cpt <= 2 ? 9 : (cpt <= 4 ? 3 : 1))) * cpt;      // (MI == 2)
            else G = BN == 16 ? (taps == 9 ? 9 : 1) * cpt : ((trunk_kind & 3) == 0 ? 18 : ((trunk_kind & 3) == 1 ? 12 : cpt));
            ph.w[TW_G] = std::min(G, kTrunkPrefetch);
            ph.w[TW_NMINE] = taps * cpt + ((p.R0 + p.R1) / ksc) / KG;
            ph.w[TW_WBYTES] = (unsigned)((N / (in_cluster ? 32 : BN)) * KG * ph.w[TW_NMINE]) * 1024u;
            pend.phases.push_back(ph);
            pend.lds = std::max(pend.lds, conv_small_lds_bytes(p, taps, BN));
            pend.flops += fl;
            pend.bytes += by;
        }
        const ConvLate late{temb_off};
        emit({[p, BN, taps, pl, late](hipStream_t st) mutable {
            late.apply(p, pl->io);
            return launch_conv_small(p, taps, BN, st);
        }, kname, fl, by}, in_trunk);
    }
    if (preact) release(act);
    *out = y;
    return 0;
}

// conv_stream.hip route: 3x3 / stride 1 convs whose output has at least 128 tiles of 32 x 8 pixels x 128 channels, or
// (the 128x8 level) of 16 x 8 pixels x 64 channels
// instance `inst` (kernels.h: kStreamInst) on pixel tile `tile` (TW = 0: the instance's only one), for a grid of [min_blocks, max_blocks] workgroups
bool Builder::stream_params_tw(const ConvArgs& a, const ConvShape& s, StreamInst inst, long long min_blocks, long long max_blocks,
                             ConvParams* q, StreamTile tile) {
    const StreamInstDesc& d = kStreamInst[inst];
    if (tile.TW == 0) tile = d.tiles[0];
    const int TW = tile.TW, TH = tile.TH;
    if (dbg() & RLDM_FLAG_NO_STREAM_REGW) return false;
    if (s.taps != 9 || a.stride != d.STR || a.pad_mode != 0 || a.out_f32_nchw || g_force_bm) return false;
    // (round 4: nearest x2 + 3x3 in its sub-pixel form -- the tiles are INPUT tiles, four parity workgroups each)
    const bool sub = d.SUB;
    ConvShape tiled = s;                    // what the tiles cut up
    if (sub) {
        if (a.up != 2 || s.R_t != 0 || s.Wout != 2 * a.x0.W || s.Hout != 2 * a.x0.H) return false;
        tiled.Wout = a.x0.W; tiled.Hout = a.x0.H;
    }
    if (tiled.Wout % TW != 0 || tiled.Hout % TH != 0) return false;
    conv_geometry(a, tiled, TW, TH, d.FH ? TH : (TH - 1) * a.stride + 3, q);      // (full-height tiles: only the tile's own rows are staged)
    if (sub) {
        q->up = 1;
        q->Wout = s.Wout; q->Hout = s.Hout;
    }
    q->st_inst = inst;
    ConvTile t;
    t.BM = 256; t.BN = 128; t.CK = 64; t.taps = 9;
    q->colb = conv_halo_col_bytes(t, TH, a.stride);
    const long long blocks = (long long)q->B * q->tiles_img * (q->N / d.bn()) * (sub ? 4 : 1);
    return supported_with(*q, a.gn != nullptr, false, [](const ConvParams& c) { return conv_stream_supported(c, 9); }) &&
           ((dbg() & RLDM_FLAG_STREAM_ANY_GRID) || (blocks >= min_blocks && blocks <= max_blocks));
}
bool Builder::stream_params(const ConvArgs& a, const ConvShape& s, ConvParams* q) {
    const int R_t = s.R_t, Hout = s.Hout;
    // the first rule that fits, in this order
    const auto fits = [&](StreamInst inst, long long min_blocks, long long max_blocks, StreamTile tile = {}) {
        return stream_params_tw(a, s, inst, min_blocks, max_blocks, q, tile);
    };
    // 256-pixel tiles when they fill the chip; else the 4-k-group instance (it re-streams the weights per 128 pixels:
    // only where its grid is about one or two rounds); else 256-pixel tiles on at least half the chip
    // (round 4) half-size workgroups, two per CU: 16 x 8 tiles x 128 channels on 4 waves where that grid is at least ~1.5 per CU
    // (UNet 256x16 level at batch >= 12, the VAE decoder's 128 / 256-channel levels), x 64 channels x 2 k-groups for the 128x8
    // level and the VAE's 64-channel level
    const int N_ = a.layer->Cout;
    const bool n128 = N_ % 128 == 0;
    // (round 4) stride 2 (Downsample2D, pad 1) on the 64-pixel x 128-channel tile with a 17 x 17 halo: the 256x16 -> 128x8 down-sampler ran on
    // the generic kernel's half-empty 256-pixel tile
    if (a.stride == 2) {
        if (!n128 || R_t != 0 || a.up != 1) return false;
        if (fits(SI_64x128_S2, kInst4MinBlocks, 512, {8, 8})) return true;
        // outputs of 4 beams (the 128x8 -> 64x4 down-sampler): 16 x 4 tiles, from 48 workgroups on
        return Hout == 4 && fits(SI_64x128_S2, 48, 512, {16, 4});
    }
    const int f2 = dbg2();
    // the 256-pixel tile's 8-wave instance: 128 channels, or 64 x 2 k-groups for layers of 64 (192, ...) output channels (round 3: the
    // VAE decoder's full-resolution level, which ran on the generic kernel at 278 us per conv)
    const StreamInst px256 = n128 ? SI_256x128 : SI_256x64;
    // (experiment, RLDM_FLAG2_STREAM_SPEC_WAVES) the 256 x 128 tile with specialised waves wherever the 8-wave 256 x 128 instance would run
    if ((f2 & RLDM_FLAG2_STREAM_SPEC_WAVES) && n128 && fits(SI_256x128_SPEC, 200, kAnyGrid)) return true;
    // (tests, RLDM_FLAG2_STREAM_64PX) the 64-pixel x 128-channel tile first, at any level it fits
    if ((f2 & RLDM_FLAG2_STREAM_64PX) && n128 && fits(SI_64x128, 192, 512)) return true;
    // (round 4) nearest x2 + 3x3 as four 2x2 convs over the input (sub-pixel form: 4 taps instead of 9 per output pixel) on the 4-wave
    // 128 x 128 tile; inputs of 4 beams: 32 x 4 tiles
    if (!(f2 & RLDM_FLAG2_STREAM_8WAVE_FULL) && a.up == 2 && n128 &&
        (fits(SI_SUB_W4, kSubMinBlocks, kAnyGrid) || (a.x0.H % 8 != 0 && fits(SI_SUB_T4_W4, kSubMinBlocks, kAnyGrid)))) return true;
    // (round 4) images of 16 beams: 8 x 16 tiles as tall as the image -- five staged pieces per thread instead of six (8 beams: 16 x 8);
    // RLDM_FLAG2_HALO_RING: the 16 x 8 tiles
    if (!(f2 & (RLDM_FLAG2_STREAM_8WAVE_FULL | RLDM_FLAG2_HALO_RING)) && n128 && (Hout == 16 || Hout == 8) && a.up == 1 &&
        fits(SI_FULLH_W4, 384, kAnyGrid, {Hout == 16 ? 8 : 16, Hout})) return true;
    if (!(f2 & RLDM_FLAG2_STREAM_8WAVE_FULL) && n128 && fits(SI_128x128_W4, 384, kAnyGrid)) return true;
    if (!(f2 & RLDM_FLAG2_STREAM_8WAVE_C64) && !n128 && fits(SI_128x64_W4, 384, kAnyGrid)) return true;
    if (fits(px256, 200, kAnyGrid)) return true;
    // (round 4) the 128x8 level: 64-pixel x 128-channel x 2-k-group tiles (8 x 8: a smaller halo, normalised once for all 128 channels,
    // half the partial sums to exchange)
    // (at the 256x16 level of small batches it breaks the clusters: -4 %; RangeDM at batch 1: +1 %, not worth a rule)
    // (one round of 8-wave workgroups: at 512 blocks -- the 256-channel up-sampler conv of the level -- two co-resident 4-wave workgroups
    // per CU win, 23.6 against 27.1 us)
    if (n128 && Hout == 8 && fits(SI_64x128, kInst4MinBlocks, 320)) return true;
    if (!(f2 & RLDM_FLAG2_STREAM_8WAVE_128X8) && fits(SI_128x64_W4, 257, 512)) return true;
    if (fits(SI_128x64, 128, 512, {16, 8})) return true;
    // images of 4 beams (nuScenes' 128 x 4 level at batch 32): the same 128-pixel instance on 32 x 4 tiles (round 3; it ran on the
    // generic kernel at 27.8 us / 257 TFLOP/s per conv: 16 % of that configuration's step)
    if (Hout % 8 != 0 && fits(SI_128x64, 128, 512, {32, 4})) return true;
    return fits(px256, 128, kAnyGrid);
}

int Builder::conv_stream(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out) {
    ConvLayer* L = a.layer;
    const int N = L->Cout;
    const Tensor& x0 = a.x0;
    if (require_gn_input(a, s.Cin_t)) return 1;
    p.dbg = kernel_dbg();
    p.ts = stamp_buf(StampSite::Conv, conv_ord - 1);
    const StreamInstDesc& d = stream_inst(p);
    const bool sub = d.SUB;
    p.ntile_n = N / d.bn() * (sub ? 4 : 1);      // (grid x: channel tiles x parities)
    Tensor y = make(x0.B, s.Wout, s.Hout, N);
    if (a.want_stats) add_stats(y, p.tiles_img * (sub ? 4 : 1));
    const double fl_ref = conv_flops(a, s);
    plan->flops += fl_ref;                  // (the network's nominal count: 9 taps)
    // what THIS launch / phase executes (the bench line's roofline is priced with it): the sub-pixel form multiplies 4 taps per output pixel
    const double fl = sub ? fl_ref * 4.0 / 9.0 : fl_ref;
    // a phase of the persistent launch (trunk.hip, variants 2 / 4): the image's tiles_img x ntile_n workgroups (16 at both
    // full-resolution levels) form a cluster on one XCD; consecutive convs of a level hand over through its L2 -- no end-of-kernel
    // write-back of the 16.8 MB outputs, no argument fetch / cold start per layer
    const int ranks_s = p.tiles_img * p.ntile_n;            // (sub-pixel form: input tiles x parities, one 128-channel tile)
    // (round 4) the 4-wave 128 x 128 instances: 32 workgroups per image, two per CU -- trunk variant 4; the 256 x 128 instance: variant 2
    const int per_cu = d.wg_per_cu();
    // (the 128x8 level's conv pairs measured slower as 2-phase launches than as two launches, 216.9 against 220.0 img/s: they
    //  stay launches)
    const bool in_stream_cluster = cluster_enabled() && ranks_s >= 2 && ranks_s <= 16 * per_cu &&
                                   trunk_grid_fits(ranks_s, x0.B, per_cu) && y.P <= kFoldAboveP && N % 128 == 0 &&
                                   d.trunk != TSF_NONE && (!sub || N == 128) && conv_stream_lds_bytes(p) <= (size_t)d.lds_cap();
    if (in_stream_cluster) trunk_begin(x0.B, ranks_s, sub ? 1 : p.ntile_n, 4, d.NW == 4 ? 4 : 2);
    else note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (sub ? L->get_subpixpacked(s.Cin_t, &pk) : L->get_streampacked(s.Cin_t, d.kgroups(), &pk)) return 1;
        bind_conv(p, a, *pk, y);
        Plan* pl = plan;
        const int temb_off = a.temb_off;
        const double by = conv_bytes(a, s);
        if (in_stream_cluster) {
            pend.phases.push_back(trunk_conv_phase(p, TK_STREAM, true, temb_off));      // (no TW_G / TW_WBYTES: variants 2 and 4 neither prefetch nor warm)
            pend.lds = std::max(pend.lds, conv_stream_lds_bytes(p));
            pend.flops += fl;
            pend.bytes += by;
        }
        const ConvLate late{temb_off};
        emit({[p, pl, late](hipStream_t st) mutable {
            late.apply(p, pl->io);
            return launch_conv_stream(p, st);
        }, "conv_stream_kernel<" + std::to_string(p.TW * p.TH) + "," + std::to_string(d.bn()) + ",CK64,taps9" + (p.stride == 2 ? ",s2" : "") + (sub ? ",sub" : "") + ">", fl, by}, in_stream_cluster);
    }
    *out = y;
    return 0;
}

// conv_regw.hip, conv_c16_kernel (round 4): the network's input layer (16 padded input channels, 128 | N, no norm / residual / time
// embedding): every weight in one wave's registers
bool Builder::c16_params(const ConvArgs& a, const ConvShape& s, ConvParams* q) {
    const int Cin_t = s.Cin_t, R_t = s.R_t, taps = s.taps, Wout = s.Wout, Hout = s.Hout;
    if ((dbg() & RLDM_FLAG_NO_STREAM_REGW) || g_force_bm || taps != 9 || a.stride != 1 || a.pad_mode != 0 || a.up != 1 || a.out_f32_nchw) return false;
    if (a.x1.valid() || a.gn || a.temb_off >= 0 || R_t != 0 || Cin_t != 16 || a.layer->Cout % 128 != 0 || Wout % 16 != 0 || Hout % 8 != 0) return false;
    conv_geometry(a, s, 16, 8, 0, q);
    q->ntile_n = q->N / 128;
    return conv_c16_supported(*q) && (long long)q->B * q->tiles_img * q->ntile_n >= 64;
}
int Builder::conv_c16(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out) {
    Tensor y = make(a.x0.B, s.Wout, s.Hout, a.layer->Cout);
    if (a.want_stats) add_stats(y, p.tiles_img);
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (a.layer->get_c16packed(&pk)) return 1;
        bind_conv(p, a, *pk, y);
        Plan* pl = plan;
        const ConvLate late{-1, a.first_of_step};
        emit({[p, pl, late](hipStream_t st) mutable {
            late.apply(p, pl->io);
            return launch_conv_c16(p, st);
        }, "conv_c16_kernel<128,128,taps9>", fl, conv_bytes(a, s)});
    }
    *out = y;
    return 0;
}

// conv_regw.hip, conv_o4_kernel (round 4): the UNet's output layer (GroupNorm + SiLU -> 3x3 over 128 channels -> <= 4 channels, fp32 NCHW + the
// scheduler step)
bool Builder::o4_params(const ConvArgs& a, const ConvShape& s, ConvParams* q) {
    const int Cin_t = s.Cin_t, R_t = s.R_t, taps = s.taps, Wout = s.Wout, Hout = s.Hout;
    if ((dbg() & RLDM_FLAG_NO_STREAM_REGW) || g_force_bm || taps != 9 || a.stride != 1 || a.pad_mode != 0 || a.up != 1 || !a.out_f32_nchw) return false;
    if (a.x1.valid() || a.temb_off >= 0 || R_t != 0 || Cin_t != 128 || a.layer->Cin != 128 || a.layer->Cout > 4 || Wout % 16 != 0 || Hout % 8 != 0) return false;
    conv_geometry(a, s, 16, 8, 0, q);
    q->ntile_n = 1;
    return supported_with(*q, a.gn != nullptr, true, conv_o4_supported) && (long long)q->B * q->tiles_img >= 64;
}
int Builder::conv_o4(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out) {
    if (require_gn_input(a, s.Cin_t)) return 1;
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (a.layer->get_streampacked(128, 2, &pk)) return 1;
        bind_conv(p, a, *pk, Tensor());         // (no bf16 output)
        Plan* pl = plan;
        const ConvLate late{-1, false, true, true};
        emit({[p, pl, late](hipStream_t st) mutable {
            late.apply(p, pl->io);
            return launch_conv_o4(p, st);
        }, "conv_o4_kernel<128,32,taps9>", fl, conv_bytes(a, s)});
    }
    *out = Tensor();
    return 0;
}

// conv_regw.hip, conv_ds2_kernel (round 4): stride-2 convs of 256 raw channels onto few pixels (the 64x4 -> 32x2 down-sampler)
bool Builder::ds2_params(const ConvArgs& a, const ConvShape& s, ConvParams* q) {
    const int Cin_t = s.Cin_t, R_t = s.R_t, taps = s.taps, Wout = s.Wout;
    if ((dbg() & RLDM_FLAG_NO_STREAM_REGW) || g_force_bm || taps != 9 || a.stride != 2 || a.pad_mode != 0 || a.up != 1 || a.out_f32_nchw) return false;
    if (a.x1.valid() || a.gn || a.temb_off >= 0 || R_t != 0 || Cin_t != 256 || a.layer->Cin != 256 || a.layer->Cout % 32 != 0 || Wout % 32 != 0) return false;
    conv_geometry(a, s, 32, 1, 0, q);
    q->ntile_n = q->N / 32;
    const long long blocks = (long long)q->B * q->tiles_img * q->ntile_n;
    return conv_ds2_supported(*q) && blocks >= 32 && blocks <= 512;      // (more: conv_stream's stride-2 instance or the generic kernel fill the chip)
}
int Builder::conv_ds2(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out) {
    Tensor y = make(a.x0.B, s.Wout, s.Hout, a.layer->Cout);
    if (a.want_stats) add_stats(y, p.tiles_img);
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (a.layer->get_streampacked(256, 2, &pk)) return 1;
        bind_conv(p, a, *pk, y);
        emit({[p](hipStream_t st) { return launch_conv_ds2(p, st); }, "conv_ds2_kernel<32,32,taps9,s2>", fl, conv_bytes(a, s)});
    }
    *out = y;
    return 0;
}

// conv_regw.hip route (round 4): 64 -> 64 channel 3x3 convs over many 16 x 8 tiles (the VAE decoder's full-resolution level) -- the weights stay
// in registers, a workgroup walks a run of tiles; RLDM_FLAG2_NO_REGW keeps them on conv_stream's per-tile instance
bool Builder::regw_params(const ConvArgs& a, const ConvShape& s, ConvParams* q) {
    const int N_ = a.layer->Cout, Cin_t = s.Cin_t, R_t = s.R_t, taps = s.taps, Wout = s.Wout, Hout = s.Hout;
    if ((dbg2() & RLDM_FLAG2_NO_REGW) || (dbg() & RLDM_FLAG_NO_STREAM_REGW) || g_force_bm || taps != 9 || a.stride != 1 || a.pad_mode != 0 || a.up != 1) return false;
    if (a.x1.valid() || a.temb_off >= 0 || Cin_t != 64 || a.layer->Cin != 64 || a.first_of_step) return false;
    if (a.out_f32_nchw ? (N_ > 4 || R_t != 0) : N_ != 64) return false;
    if (R_t != 0 && !(a.layer->sc_identity && R_t == 64 && a.r0.valid() && a.r0.C == 64)) return false;
    if (Wout % 16 != 0 || Hout % 8 != 0) return false;
    conv_geometry(a, s, 16, 8, 10, q);
    ConvTile t;
    t.BM = 256; t.BN = 128; t.CK = 64; t.taps = 9;
    q->colb = conv_halo_col_bytes(t, 8, 1);
    q->exp = (dbg2() & RLDM_FLAG2_REGW_CAP8) ? 8 : 0;      // (tests: at most 8 team runs, so that small images give runs of several tiles)
    return supported_with(*q, a.gn != nullptr, a.out_f32_nchw, conv_regw_supported);
}
int Builder::conv_regw(const ConvArgs& a, const ConvShape& s, ConvParams p, Tensor* out) {
    if (require_gn_input(a, s.Cin_t)) return 1;
    p.dbg = kernel_dbg();
    p.ts = g_ts_buf;
    p.ntile_n = 1;
    Tensor y;
    if (!a.out_f32_nchw) {
        y = make(a.x0.B, s.Wout, s.Hout, a.layer->Cout);
        if (a.want_stats) add_stats(y, conv_regw_partials(p));
    }
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (a.layer->get_streampacked(s.Cin_t, 1, &pk)) return 1;
        bind_conv(p, a, *pk, y);
        Plan* pl = plan;
        const ConvLate late{-1, false, a.out_f32_nchw};          // (io.out without the scheduler step: the kernel has none)
        emit({[p, pl, late](hipStream_t st) mutable {
            RLDM_REQUIRE(!late.f32_out || pl->io.sch.coef_table == nullptr, "conv_regw: a scheduler step fused into this output layer");
            late.apply(p, pl->io);
            return launch_conv_regw(p, st);
        }, std::string("conv_regw_kernel<128,") + (late.f32_out ? "32" : "64") + ",taps9>", fl, conv_bytes(a, s, 1, false)});
    }
    *out = y;
    return 0;
}

// Statistics of a tensor with many pixel tiles per image are folded once, by one small launch, instead of by every
// workgroup of every consumer (gn_fold_kernel).
int Builder::fold_stats(Tensor& y) {
    if (!y.valid() || y.P <= kFoldAboveP) return 0;
    const size_t raw_off = y.st_off, raw_bytes = y.st_bytes();
    const int rawP = y.P;
    add_stats(y, 2);
    note_launch();
    if (!dry) {
        GnFoldParams g;
        g.part = ptr<float2>(raw_off);
        g.out = ptr<float2>(y.st_off);
        g.B = y.B; g.P = rawP; g.C = y.C;
        plan->ops.push_back({[g](hipStream_t s) { return launch_gn_fold(g, s); }, "gn_fold_kernel", 0.0, (double)raw_bytes});
    }
    arena.release(raw_off, raw_bytes);
    return 0;
}

// y = conv(...) ; consumes nothing (callers release inputs)
int Builder::conv(const ConvArgs& a0, Tensor* out) {
    ConvArgs a = a0;
    const int ord = conv_ord++;
    ConvLayer* L = a.layer;
    RLDM_REQUIRE(L != nullptr, "internal: missing conv layer");
    Tensor view;
    if (vp && !recording && take_view(a.gn, &view)) {
        a.x0 = view; a.x1 = Tensor(); a.gn = nullptr; a.silu = 0;
    }
    const ConvShape s = conv_shape(a);
    if (recording && vp) {
        // as a consumer: could this conv read cat[x0, x1] already normalised + activated?  (3x3 on the conv_small route)
        ConvArgs c = a;
        c.x0.C = s.Cin_t; c.x1 = Tensor(); c.gn = nullptr; c.silu = 0;
        if (a.gn) record_consumer(a.gn, a.x0, a.x1, a.silu, s.taps == 9 && small_route(c, s), a.groups, a.eps);
        // as a producer: with one tile per image, whether its own input arrives raw (statistics) or pre-activated
        ConvArgs o = a, oc = c;
        o.own_image = oc.own_image = true;
        if ((int)vp->can_emit.size() <= ord) vp->can_emit.resize(ord + 1, 0);
        if ((int)vp->out_c.size() <= ord) vp->out_c.resize(ord + 1, 0);
        vp->out_c[ord] = L->Cout;
        vp->can_emit[ord] = !(dbg() & RLDM_FLAG_CONSUMER_GN) && !a.out_f32_nchw && small_route(o, s) && (!a.gn || small_route(oc, s));
    } else if (vp) {
        auto it = vp->emit.find(ord);
        cur_emit = (it != vp->emit.end() && !it->second.empty()) ? &it->second : nullptr;
        // one tile per image: to normalise for the consumers, and (input ready, nothing to fold) to be a trunk phase
        a.own_image = cur_emit != nullptr ||
                      (!a.gn && ord < (int)vp->can_emit.size() && vp->can_emit[ord] && !a.x1.valid());
    }
    const size_t ops_before = plan->ops.size(), ph_before = pend.standalone.size();
    if (conv_route(a, s, out)) return 1;
    if (!dry) {
        for (size_t i = ops_before; i < plan->ops.size(); ++i) plan->ops[i].tag += L->name + " ";
        for (size_t i = ph_before; i < pend.standalone.size(); ++i) pend.standalone[i].tag += L->name + " ";
    }
    cur_emit = nullptr;
    if (view.valid()) release(view);
    out->prod = ord;
    if (out->valid()) live[out->id] = *out;
    return fold_stats(*out);
}
// the first route that admits the conv, in this order; its *_params has filled the ConvParams the emitter goes on with
int Builder::conv_route(const ConvArgs& a, const ConvShape& s, Tensor* out) {
    ConvLayer* L = a.layer;
    RLDM_REQUIRE(s.Cin_t >= L->Cin, "conv " + L->name + ": input tensor has fewer channels than the weights");
    RLDM_REQUIRE(s.Cin_t % 16 == 0, "conv " + L->name + ": input channels must be a multiple of 16");
    RLDM_REQUIRE(s.R_t == L->R, "conv " + L->name + ": residual sources do not match the layer's residual phase");
    RLDM_REQUIRE((a.x0.W * a.up) % a.stride == 0 && (a.x0.H * a.up) % a.stride == 0, "conv " + L->name + ": odd size under stride 2");
    RLDM_REQUIRE(s.R_t == 0 || (a.r0.W == s.Wout && a.r0.H == s.Hout), "conv " + L->name + ": residual resolution mismatch");
    // (conv_in stays off the routes that cannot advance the sampler's step index: it is the step's first launch)
    const bool first = a.first_of_step;
    ConvParams p;
    bool epi_res = false;
    int bn = 0;
    if (!first && small_route(a, s, &p, &epi_res, &bn)) return conv_small(a, s, p, epi_res, bn, out);
    if (c16_params(a, s, &p)) return conv_c16(a, s, p, out);
    if (o4_params(a, s, &p)) return conv_o4(a, s, p, out);
    if (!first && ds2_params(a, s, &p)) return conv_ds2(a, s, p, out);
    if (regw_params(a, s, &p)) return conv_regw(a, s, p, out);
    if (!first && stream_params(a, s, &p)) return conv_stream(a, s, p, out);
    return conv_generic(a, s, out);
}

// conv_igemm.hip: the implicit-GEMM kernel every other conv runs on, on the tile choose_tile picks
int Builder::conv_generic(const ConvArgs& a, const ConvShape& s, Tensor* out) {
    ConvLayer* L = a.layer;
    const Tensor& x0 = a.x0;
    const int N = L->Cout, Wout = s.Wout, Hout = s.Hout;
    const TileChoice tc = choose_tile(x0.B, Wout, Hout, a.stride, N, s.Cin_t, x0.C, s.R_t, a.r0.valid() ? a.r0.C : 0, s.taps,
                                      a.out_f32_nchw, a.gn != nullptr);
    const ConvTile tile = tc.tile;
    RLDM_REQUIRE(conv_tile_supported(tile), "conv " + L->name + ": no kernel instance");
    RLDM_REQUIRE((tc.TH & (tc.TH - 1)) == 0, "conv " + L->name + ": pixel tile height must be a power of two");
    RLDM_REQUIRE(Wout % tc.TW == 0 && Hout % tc.TH == 0, "conv " + L->name + ": size not tileable (powers of two expected)");

    ConvParams p;
    conv_geometry(a, s, tc.TW, tc.TH, (tc.TH - 1) * a.stride + (L->ksize == 3 ? 3 : 1), &p);
    p.colb = conv_halo_col_bytes(tile, tc.TH, a.stride);
    p.dbg = kernel_dbg();
    p.ts = stamp_buf(StampSite::Conv, conv_ord - 1);
    p.ksplit = tc.ksplit;
    p.ntile_n = (N + tile.BN - 1) / tile.BN;
    const long long tiles = (long long)x0.B * p.tiles_img * p.ntile_n;

    Tensor y;
    if (!a.out_f32_nchw) {
        y = make(x0.B, Wout, Hout, N);
        if (a.want_stats) add_stats(y, p.tiles_img);
    }
    if (require_gn_input(a, s.Cin_t)) return 1;
    size_t slab_off = 0, slab_bytes = 0;
    int ticket_base = 0;
    if (tc.ksplit > 1) {
        slab_bytes = (size_t)tiles * tc.ksplit * tile.BM * tile.BN * sizeof(float);
        slab_off = arena.alloc(slab_bytes);
        ticket_base = tickets;
        tickets += (int)tiles;
    }
    const double fl = conv_flops(a, s);
    plan->flops += fl;
    note_launch();
    if (!dry) {
        ConvLayer::Packed* pk = nullptr;
        if (L->get_packed(tile.BN, tile.CK, s.Cin_t, &pk)) return 1;
        bind_conv(p, a, *pk, y);
        if (tc.ksplit > 1) {
            p.slab = ptr<float>(slab_off);
            p.ticket = ticket_ptr + ticket_base;
        }
        Plan* pl = plan;
        const ConvLate late{a.temb_off, a.first_of_step, a.out_f32_nchw, a.out_f32_nchw};
        const std::string kname = "conv_igemm_kernel<" + std::to_string(tile.BM) + "," + std::to_string(tile.BN) +
                                  ",CK" + std::to_string(tile.CK) + ",taps" + std::to_string(tile.taps) + ">";
        emit({[p, tile, pl, late](hipStream_t st) mutable {
            late.apply(p, pl->io);
            return launch_conv(tile, p, st);
        }, kname, fl, conv_bytes(a, s)});
    }
    if (tc.ksplit > 1) arena.release(slab_off, slab_bytes);
    *out = y;
    return 0;
}

int build_plan(Plan* plan, int temb_ld, const std::function<int(Builder&)>& walk, int* launches, int concurrent_plans, bool count_only) {
    PlanFlagScope scope(plan->flags);
    // pass 0 records which GroupNorms could be applied by the producers of their inputs (ViewPlan)
    ViewPlan vplan;
    {
        Builder rec;
        rec.plan = plan;
        rec.dry = true;
        rec.recording = true;
        rec.vp = &vplan;
        rec.temb_ld = temb_ld;
        rec.concurrent_plans = concurrent_plans;
        if (walk(rec)) return 1;
        vplan.decide();
        // tests (RLDM_FLAG_OWN_IMAGE_COPIES): every conv that could normalise for a consumer writes two copies nobody reads (identity
        // affine, SiLU on) -- the own-image tile + epilogue on single-conv plans
        if (!count_only && (dbg() & RLDM_FLAG_OWN_IMAGE_COPIES)) {      // (a count is of the network as it is)
            static std::map<int, std::unique_ptr<NormParams>> dummies;
            for (int ord = 0; ord < (int)vplan.can_emit.size(); ++ord) {
                if (!vplan.can_emit[ord] || vplan.emit.count(ord) || vplan.out_c[ord] % 32 != 0) continue;
                const int C = vplan.out_c[ord];
                for (int i = 0; i < 2; ++i) {
                    auto& d = dummies[C * 4 + i];
                    if (!d) {
                        d = std::make_unique<NormParams>();
                        d->C = C;
                        std::vector<float> one(C, 1.f), zero(C, 0.f);
                        if (upload(d->gamma, one.data(), C * 4) || upload(d->beta, zero.data(), C * 4)) return 1;
                    }
                    vplan.emit[ord].push_back({d.get(), 0, C, 1, 32, 1e-5f});
                }
            }
        }
        plan->flops = 0;
    }
    Builder dry;
    dry.plan = plan;
    dry.dry = true;
    dry.temb_ld = temb_ld;
    dry.concurrent_plans = concurrent_plans;
    dry.vp = &vplan;
    if (walk(dry)) return 1;
    if (dry.flush_trunk()) return 1;
    if (launches) *launches = dry.launches;
    if (count_only) return 0;
    if (plan->arena.alloc(dry.arena.peak + 256)) return 1;
    if (plan->tickets.alloc((size_t)std::max(1, dry.tickets) * sizeof(int))) return 1;
    RLDM_HIP_CHECK(hipMemset(plan->tickets.p, 0, plan->tickets.bytes));
    plan->flops = 0;
    plan->ops.clear();
    Builder real;
    real.plan = plan;
    real.dry = false;
    real.base = plan->arena.as<char>();
    real.ticket_ptr = plan->tickets.as<int>();
    real.temb_ld = temb_ld;
    real.concurrent_plans = concurrent_plans;
    real.vp = &vplan;
    if (walk(real)) return 1;
    if (real.flush_trunk()) return 1;
    if (getenv("RLDM_PRINT_PLAN")) {                 // tuning aid: the launch list of every plan built
        fprintf(stderr, "plan B=%d %dx%d: %zu launches\n", plan->B, plan->W, plan->H, plan->ops.size());
        for (size_t i = 0; i < plan->ops.size(); ++i)
            fprintf(stderr, "  %3zu %-64s %8.3f GFLOP %8.2f MB  %s\n", i, plan->ops[i].name.c_str(), plan->ops[i].flops * 1e-9,
                    plan->ops[i].bytes * 1e-6, plan->ops[i].tag.c_str());
    }
    return 0;
}

}  // namespace rldm

using namespace rldm;

// ---- the routing state's setters ------------------------------------------------------------------------------------
extern "C" {

int rldm_debug_set_flags2(int flags) {
    g_dbg_flags2 = flags;
    return 0;
}
int rldm_debug_set_flags(int flags) {
    g_dbg_flags = flags;
    return 0;
}

// enable (host_out == NULL: allocate + zero) or read back (host_out = 256 x u64) the in-kernel timestamps of the conv kernel
static constexpr int kTsBlocks = 2048;          // per-workgroup [start, end] s_memrealtime pairs behind the 256 stamps
int rldm_debug_timestamps(unsigned long long* host_out) {
    if (!g_ts_buf) {
        RLDM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g_ts_buf), (256 + 2 * kTsBlocks) * 8));
        RLDM_HIP_CHECK(hipMemset(g_ts_buf, 0, (256 + 2 * kTsBlocks) * 8));
    }
    if (host_out) {
        RLDM_HIP_CHECK(hipDeviceSynchronize());
        RLDM_HIP_CHECK(hipMemcpy(host_out, g_ts_buf, 256 * 8, hipMemcpyDeviceToHost));
        RLDM_HIP_CHECK(hipMemset(g_ts_buf, 0, 256 * 8));
    }
    return 0;
}
// ABLATE builds of conv_stream.hip: [start, end] of every workgroup (first 2048) of the last launch on the 100 MHz
// s_memrealtime counter, which all XCDs share -- the spread of the starts / ends is the launch's dispatch and tail skew
int rldm_debug_block_times(unsigned long long* host_out, int nblocks) {
    RLDM_REQUIRE(host_out && nblocks >= 1 && nblocks <= kTsBlocks, "block times: 1..2048 blocks");
    RLDM_REQUIRE(g_ts_buf != nullptr, "block times: call rldm_debug_timestamps(NULL) first");
    RLDM_HIP_CHECK(hipDeviceSynchronize());
    RLDM_HIP_CHECK(hipMemcpy(host_out, g_ts_buf + 256, (size_t)nblocks * 16, hipMemcpyDeviceToHost));
    RLDM_HIP_CHECK(hipMemset(g_ts_buf + 256, 0, 2 * kTsBlocks * 8));
    return 0;
}

int rldm_debug_force_tile(int BM, int BN, int ksplit) {
    g_force_bm = BM;
    g_force_bn = BN;
    g_force_ks = ksplit;
    return 0;
}

}  // extern "C"
