// The sampler: lanes (independent slices of the batch with their own plans, streams and captured step graphs), the HIP-graph
// captured sampling loop (ldm/pipelines.py:353-367), the scheduler-step entry points and the step-graph trace.
#include "runtime.h"

using namespace rldm;

static constexpr int kGraphSteps = 10;          // sampler steps per captured graph (at most; a divisor of the step count)

// =================================================================================================================
// sampler
// =================================================================================================================
// One lane = an independent slice of the batch with its own plans, buffers, stream and captured graphs.  Whole samples
// never interact, so the lanes' 50-step chains run concurrently on separate streams: the low-resolution UNet levels
// launch far fewer workgroups than the chip has CUs, and a second (third, fourth) chain fills the idle ones.
// the four extra tensors of rldm_sample_guided (null for an unguided sampler)
struct GuidedIO {
    const float* known = nullptr;
    const float* mask = nullptr;
    const float* known_noise = nullptr;
    const float* renoise_noise = nullptr;
    bool operator==(const GuidedIO& o) const {
        return known == o.known && mask == o.mask && known_noise == o.known_noise && renoise_noise == o.renoise_noise;
    }
};
// One rldm_sample* call: what its entry point was given, handed by const reference to everything that works for the call (the
// fall-back re-entry of sample_impl included).  Nothing of it outlives the call on the sampler or its lanes.
struct SampleCall {
    const float* x_T = nullptr;                     // null (rng only): drawn from the generator as well
    const float* step_noise = nullptr;
    const float* cond = nullptr;
    GuidedIO gio;
    float* images = nullptr;
    float* latents_out = nullptr;
    void* stream = nullptr;
    bool rng_on = false;                            // the call draws its noise on the device (rldm_sample_rng): its generator
    uint64_t rng_seed = 0;                          // (the noise tensors are then the lanes' row buffers, read with stride 0)
    uint32_t rng_draw = 0, rng_offset = 0;
};

static DevBuf g_trace;                              // rldm_debug_graph_trace: 4096 timestamps
static const Plan* g_trace_plan = nullptr;          // ... of this plan, a live lane's uplan: SamplerLane::drop_uplan clears it

struct SamplerLane {
    int b0 = 0, nb = 0;                             // samples [b0, b0 + nb) of the batch
    std::unique_ptr<Plan> uplan;                    // private UNet plan (graph-baked pointers)
    std::unique_ptr<Plan> dplan;                    // private VAE decode plan
    DevBuf x, eps, cond, step, image;
    DevBuf hist;                                    // RLDM_SAMPLER_DPMSOLVER: the previous step's x0 (sized like x); RLDM_SAMPLER_UNIPC: the
    DevBuf last;                                    // three previous steps' x0 ([3] like x) and the previous step's corrected sample
    // rldm_sample_rng / rldm_sample_guided_rng: {seed low, seed high, draw, sample offset} of the call, and one row of noise (sized
    // like x) per purpose the rows need -- filled at the head of every step, read by the scheduler step with stride 0 like hist
    DevBuf rng_record, rng_step, rng_known, rng_renoise;
    hipStream_t stream = nullptr;
    hipEvent_t ev_out = nullptr;
    hipGraphExec_t step_graph = nullptr, decode_graph = nullptr;
    int graph_steps = 1;                            // sampler steps captured in step_graph
    bool fused_tail = true;                         // scheduler step in conv_out's epilogue, step index advanced by pack_input
    const float* captured_noise = nullptr;
    GuidedIO guided, captured_guided;               // guided sampler: this call's tensors (offset to the lane) / those the graph holds
    long long n_latent = 0, n_image = 0, n_cond = 0;
    int* check_host = nullptr;                      // pinned: the persistent launches' self-check word of the last call (copied behind its
    bool check_pending = false;                     // last launch; read by rldm_sampler_status, the next call or the destructor)
    std::atomic<bool> call_recorded{false};         // ev_out has been recorded at least once (read by other samplers' threads: in_flight)
    void drop_uplan() {
        if (g_trace_plan == uplan.get()) g_trace_plan = nullptr;
        uplan.reset();
    }
    ~SamplerLane() {
        drop_uplan();
        if (check_host) (void)hipHostFree(check_host);
        if (step_graph) (void)hipGraphExecDestroy(step_graph);
        if (decode_graph) (void)hipGraphExecDestroy(decode_graph);
        if (ev_out) (void)hipEventDestroy(ev_out);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct rldm_sampler {
    rldm_unet* unet = nullptr;
    rldm_vae* vae = nullptr;
    rldm_sampler_config cfg;
    DevBuf coef, temb_tab, t_dev;                   // shared, read-only after creation
    std::vector<std::unique_ptr<SamplerLane>> lanes;
    hipEvent_t ev_in = nullptr;
    long long n_latent = 0, n_image = 0;            // whole batch
    uint64_t unet_gen = 0, vae_gen = 0;             // generations of the weights the lanes' plans and graphs were built on
    int plan_flags = 0;                             // routing options of this sampler's plans (rldm_sampler_config::plan_flags | fall-backs)
    int device = 0;
    std::atomic<hipStream_t> last_caller{nullptr};  // stream of the last rldm_sample call (ordering against other samplers' calls; read
                                                    // by other samplers' host threads under g_samplers_mu -- atomics, not plain fields)
    std::atomic<bool> shared_mark{false};           // another sampler found THIS one in flight beside its own call: drop the persistent
                                                    // launches at the next call instead of meeting that sampler's launches again
    int latched_error = 0;                          // self-check code of a call whose pending word was read while the plans were rebuilt
    int inject_error = 0;                           // tests: rldm_debug_inject_trunk_error (one shot)
    int captures = 0;                               // step graphs captured so far (rldm_debug_sampler_captures)
    bool needs_known_noise = false, needs_renoise_noise = false;   // guided: some row has kb != 0 / (ra, rb) != (1, 0)
    bool has_persistent() const {
        for (auto& ln : lanes)
            if (ln->uplan && ln->uplan->trunk_error.p) return true;
        return false;
    }
    bool in_flight() const {                        // some lane's last call has not finished
        for (auto& ln : lanes)
            if (ln->ev_out && ln->call_recorded && hipEventQuery(ln->ev_out) == hipErrorNotReady) return true;
        return false;
    }
    ~rldm_sampler();
};

// Live samplers of the process: a sampler whose plans hold persistent launches (trunk.hip: 256 co-resident workgroups that wait for
// each other) must have the device to itself while they run.  rldm_sample looks for another sampler's call still in flight on a
// DIFFERENT caller stream (same stream: ordered behind it) and, if there is one, runs -- from then on -- one launch per layer.
static std::mutex g_samplers_mu;
static std::vector<rldm_sampler*> g_samplers;

rldm_sampler::~rldm_sampler() {
    {
        std::lock_guard<std::mutex> lk(g_samplers_mu);
        g_samplers.erase(std::remove(g_samplers.begin(), g_samplers.end(), this), g_samplers.end());
    }
    for (auto& ln : lanes) {                        // the last call of a run is never followed by another: say so here
        if (ln->check_pending && ln->ev_out && hipEventSynchronize(ln->ev_out) == hipSuccess && ln->check_host && *ln->check_host != 0)
            fprintf(stderr, "librangeldm_hip: the LAST rldm_sample call of a sampler failed the self-check of its persistent launches "
                            "(code %d): its images were NaN-marked\n", *ln->check_host);
    }
    lanes.clear();
    if (ev_in) (void)hipEventDestroy(ev_in);
}

// (RLDM_FLAG_SCHED_LAUNCH at sampler creation keeps the scheduler step and the step counter as launches of their own; a guided sampler
//  and RLDM_SAMPLER_UNIPC always run that way)

int rldm::sched_mode_word(int sampler_mode, int prediction_type) {
    if (sampler_mode == RLDM_SAMPLER_UNIPC) return -1;     // no 5-wide row, no word: launch_sched_step refuses it
    return (sampler_mode == RLDM_SAMPLER_DDIM ? 0 : 1) | (prediction_type << 1) | (sampler_mode == RLDM_SAMPLER_DPMSOLVER ? kSchedMultistep : 0);
}
static int sampler_sched_mode(const rldm_sampler* s) { return sched_mode_word(s->cfg.mode, s->cfg.prediction_type); }

void rldm::fill_sched_fuse(SchedFuse& f, const float* coef_table, const int* step_ptr, const float* x, float* x_prev, int mode,
                           NoiseSrc noise, bf16_t* pack, int pack_ld) {
    f.coef_table = coef_table;
    f.step_ptr = step_ptr;
    f.x = x;
    f.x_prev = x_prev;
    f.mode = mode;
    f.noise = noise.p;
    f.noise_step_stride = noise.step_stride;
    f.pack = pack;
    f.pack_ld = pack_ld;
}

// a lane's scheduler step reads: a multistep sampler its x0 history, the same elements every step (no per-call tensor); any other the
// call's `noise`, already offset to the lane's first sample -- the lane's own row buffer (rng: refilled every step) or the caller's
// [steps][whole batch][...] tensor
static NoiseSrc lane_noise_src(const rldm_sampler* s, const SamplerLane* ln, const float* noise, bool own_noise) {
    if (s->cfg.mode == RLDM_SAMPLER_DPMSOLVER) return {ln->hist.as<float>(), 0};
    if (s->cfg.mode == RLDM_SAMPLER_UNIPC) return {nullptr, 0};     // (its step takes its state by name: sampler_enqueue_step)
    return {noise, own_noise ? 0 : s->n_latent};
}

// a fill of `out` from the call's generator for the lane's samples (purpose 0 / row 0: x_T; the steps' rows set the rest)
static RngFillParams lane_rng_fill(const SamplerLane* ln, float* out) {
    RngFillParams rp{};
    rp.out = out;
    rp.per_sample = ln->n_latent / ln->nb;
    rp.B = ln->nb;
    rp.record = ln->rng_record.as<unsigned>();
    rp.sample0 = (unsigned)ln->b0;
    return rp;
}

// x_T (just copied into the lane's x) as conv_in's input: once per call when the steps' pack_input launch is fused into conv_out
static int sampler_pack_x(rldm_sampler* s, SamplerLane* ln, hipStream_t st) {
    const PlanIO& io = ln->uplan->io;
    if (!io.pack_fused) return 0;
    const auto& uc = s->unet->cfg;
    PackInputParams p{};
    p.x = io.sample; p.cx = io.sample_channels; p.scale = io.sample_scale;
    p.pos_encoding = io.pos_encoding;
    p.cond = io.cond; p.cc = io.cond_channels;
    p.B = ln->nb; p.W = uc.sample_w; p.H = uc.sample_h; p.Cpad = io.xin_ld;
    p.out = io.xin;
    p.step_inc = nullptr;
    return launch_pack_input(p, st);
}

static int sampler_enqueue_step(rldm_sampler* s, SamplerLane* ln, const SampleCall& c, const float* noise, hipStream_t st) {
    const bool fused = ln->fused_tail;
    const NoiseSrc src = lane_noise_src(s, ln, noise, c.rng_on);
    // (the rest of io.sch / io.step_inc: sampler_build_plans)
    if (fused) {
        ln->uplan->io.sch.noise = src.p;
        ln->uplan->io.sch.noise_step_stride = src.step_stride;
    }
    if (c.rng_on) {
        // the row this step's scheduler launch reads: the step word itself where it is advanced AFTER that launch (it starts at 0),
        // the word + 1 with the fused tail (it starts at -1 and the step's first launch, which follows this one, advances it)
        RngFillParams rp = lane_rng_fill(ln, nullptr);
        rp.step_ptr = ln->step.as<int>();
        rp.row = fused ? 1u : 0u;
        const float* bufs[3] = {noise, ln->guided.known_noise, ln->guided.renoise_noise};
        for (int k = 0; k < 3; ++k) {
            if (!bufs[k]) continue;
            rp.out = const_cast<float*>(bufs[k]);
            rp.purpose = 1u + k;
            if (launch_rng_fill(rp, st)) return 1;
        }
    }
    if ((dbg_process() | s->plan_flags) & RLDM_FLAG_GRAPH_TRACE) {
        if (!g_trace.p) {
            if (g_trace.alloc(4096 * 8)) return 1;
            RLDM_HIP_CHECK(hipMemset(g_trace.p, 0, 4096 * 8));
        }
        g_trace_plan = ln->uplan.get();
        if (ln->uplan->run_stamped(st, g_trace.as<unsigned long long>(), 4096)) return 1;
    } else if (ln->uplan->run(st)) return 1;
    if (fused) return 0;
    if (s->cfg.mode == RLDM_SAMPLER_UNIPC) {
        // row *step of the [steps][12] table on the lane's own state; row 0 has no corrector and reads none of it, so a call starts
        // clean on whatever the previous call (or the warm-up step) left there
        UniPCParams up;
        memset(&up, 0, sizeof(up));
        up.pred = s->cfg.prediction_type;
        up.coef_table = s->coef.as<float>();
        up.step_ptr = ln->step.as<int>();
        up.out = ln->eps.as<float>();
        up.x = ln->x.as<float>();
        up.last = ln->last.as<float>();
        up.hist = ln->hist.as<float>();
        up.x_prev = ln->x.as<float>();
        up.n = ln->n_latent;
        if (launch_sched_unipc_step(up, st)) return 1;
        return launch_step_counter(ln->step.as<int>(), 0, 1, st);
    }
    SchedParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.mode = sampler_sched_mode(s);
    sp.coef_table = s->coef.as<float>();
    sp.step_ptr = ln->step.as<int>();
    sp.eps = ln->eps.as<float>();
    sp.x = ln->x.as<float>();
    sp.noise = src.p;
    sp.noise_step_stride = src.step_stride;
    sp.x_prev = ln->x.as<float>();
    sp.n = ln->n_latent;
    if (s->cfg.guided) {
        // the guided step stands where the scheduler step stands: same row index, rows of 9, two more per-row noise tensors
        const auto& uc = s->unet->cfg;
        GuidedSchedParams gp;
        memset(&gp, 0, sizeof(gp));
        gp.s = sp;
        gp.known = ln->guided.known;
        gp.mask = ln->guided.mask;
        gp.known_noise = ln->guided.known_noise;
        gp.renoise_noise = ln->guided.renoise_noise;
        gp.spatial = (long long)uc.sample_w * uc.sample_h;
        gp.per_sample = gp.spatial * uc.out_channels;
        if (launch_sched_guided_step(gp, st)) return 1;
    } else if (launch_sched_step(sp, st)) return 1;
    return launch_step_counter(ln->step.as<int>(), 0, 1, st);
}

// (Re)build everything of a sampler that is baked on the models' device weights: the time-embedding table, every lane's
// UNet / decode plan (weight pointers, packed images) and -- by dropping them -- the captured graphs.  Called at creation
// and again by rldm_sample when rldm_unet_finalize / rldm_vae_finalize ran since (load_state_dict on a model a pipeline
// already sampled with: the old graphs would replay over freed weight buffers).
static int sampler_build_plans(rldm_sampler* s) {
    rldm_unet* unet = s->unet;
    rldm_vae* vae = s->vae;
    RLDM_REQUIRE(unet->params.finalized, "unet not finalized (set_param without rldm_unet_finalize)");
    RLDM_REQUIRE(!vae || vae->params.finalized, "vae not finalized (set_param without rldm_vae_finalize)");
    const auto& uc = unet->cfg;
    const int W = uc.sample_w, H = uc.sample_h;
    for (auto& lnp : s->lanes) RLDM_HIP_CHECK(hipStreamSynchronize(lnp->stream));
    if (s->temb_tab.alloc((size_t)s->cfg.num_steps * unet_temb_ld(unet) * 4)) return 1;
    if (unet_temb(unet, s->t_dev.as<float>(), s->cfg.num_steps, s->temb_tab.as<float>(), nullptr)) return 1;
    RLDM_HIP_CHECK(hipStreamSynchronize(nullptr));
    for (auto& lnp : s->lanes) {
        SamplerLane* ln = lnp.get();
        if (ln->step_graph) { (void)hipGraphExecDestroy(ln->step_graph); ln->step_graph = nullptr; }
        if (ln->decode_graph) { (void)hipGraphExecDestroy(ln->decode_graph); ln->decode_graph = nullptr; }
        ln->captured_noise = nullptr;
        ln->captured_guided = GuidedIO();
        ln->drop_uplan();
        ln->dplan.reset();
        const int prc = unet_make_plan(unet, ln->nb, &ln->uplan, nullptr, s->plan_flags, (int)s->lanes.size());
        // (the lane streams were synchronised above: a pending self-check word of the previous, asynchronous call has landed -- keep it)
        if (ln->check_pending && ln->check_host && *ln->check_host != 0) s->latched_error = *ln->check_host;
        ln->check_pending = false;
        if (prc) return 1;
        PlanIO& io = ln->uplan->io;
        io.sample = ln->x.as<float>();
        io.sample_channels = uc.out_channels;
        io.pos_encoding = s->cfg.pos_encoding;
        io.cond = s->cfg.cond_channels ? ln->cond.as<float>() : nullptr;
        io.cond_channels = s->cfg.cond_channels;
        io.out = ln->eps.as<float>();
        io.temb = s->temb_tab.as<float>();
        io.step_ptr = ln->step.as<int>();
        io.temb_rows_per_step = 1;
        io.temb_per_sample = 0;
        // (a guided sampler blends AFTER the scheduler step: the input conv_out's epilogue would pack for the next step would be stale)
        // (UniPC's step reads and shifts more state than conv_out's epilogue carries: a launch of its own)
        ln->fused_tail = !((dbg_process() | s->plan_flags) & RLDM_FLAG_SCHED_LAUNCH) && !s->cfg.guided && s->cfg.mode != RLDM_SAMPLER_UNIPC;
        if (ln->fused_tail) {
            // the scheduler step rides in conv_out's epilogue, the step index is advanced by pack_input: 2 launches per step fewer
            // ... and the next step's conv_in input: no pack_input launch inside the steps
            io.pack_fused = io.xin && io.sample_scale == 1.f;
            // (the noise tensor is the call's: sampler_enqueue_step)
            fill_sched_fuse(io.sch, s->coef.as<float>(), ln->step.as<int>(), ln->x.as<float>(), ln->x.as<float>(), sampler_sched_mode(s),
                            lane_noise_src(s, ln, nullptr, false), io.pack_fused ? io.xin : nullptr, io.pack_fused ? io.xin_ld : 0);
            io.step_inc = ln->step.as<int>();
        }
        if (vae) {
            if (vae_make_plan(vae, ln->nb, W, H, false, &ln->dplan, s->plan_flags)) return 1;
            PlanIO& d = ln->dplan->io;
            d.sample = ln->x.as<float>();
            d.sample_channels = vae->cfg.z_channels;
            d.sample_scale = 1.0f / vae->cfg.scaling_factor;      // latents / scaling_factor, ldm/pipelines.py:365
            d.out = ln->image.as<float>();
        }
    }
    s->unet_gen = unet->generation;
    s->vae_gen = vae ? vae->generation : 0;
    return 0;
}

static int capture(hipStream_t st, const std::function<int()>& body, hipGraphExec_t* exec) {
    RLDM_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return 1;
    }
    RLDM_HIP_CHECK(e);
    if (*exec) {
        (void)hipGraphExecDestroy(*exec);
        *exec = nullptr;
    }
    RLDM_HIP_CHECK(hipGraphInstantiate(exec, g, nullptr, nullptr, 0));
    RLDM_HIP_CHECK(hipGraphDestroy(g));
    return 0;
}

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

// ---- scheduler steps ----------------------------------------------------------------------------------------------
static int sched_step(int mode, const float coef[5], const float* eps, const float* x, const float* noise, float* x_prev,
                      int64_t n, void* stream) {
    RLDM_REQUIRE(coef && eps && x && x_prev, "null argument");
    RLDM_REQUIRE(coef[4] == 0.f || noise != nullptr, "sigma != 0 requires a noise tensor");
    SchedParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.mode = mode;
    for (int i = 0; i < 5; ++i) sp.coef[i] = coef[i];
    sp.eps = eps; sp.x = x; sp.noise = noise; sp.x_prev = x_prev; sp.n = n;
    return launch_sched_step(sp, reinterpret_cast<hipStream_t>(stream));
}
int rldm_sched_ddim_step(const float coef[5], const float* eps, const float* x, const float* noise, float* x_prev,
                         int64_t n, void* stream) {
    return sched_step(0, coef, eps, x, noise, x_prev, n, stream);
}
int rldm_sched_ddpm_step(const float coef[5], const float* eps, const float* x, const float* noise, float* x_prev,
                         int64_t n, void* stream) {
    return sched_step(1, coef, eps, x, noise, x_prev, n, stream);
}
int rldm_sched_dpmsolver_step(int prediction_type, const float coef[5], const float* model_output, const float* x,
                              float* x0_history, float* x_prev, int64_t n, void* stream) {
    RLDM_REQUIRE(prediction_type >= RLDM_PRED_EPSILON && prediction_type <= RLDM_PRED_SAMPLE, "unknown prediction type");
    RLDM_REQUIRE(x0_history != nullptr, "null argument");
    RLDM_REQUIRE(x0_history != x_prev && x0_history != x && x0_history != model_output, "x0_history must not alias another tensor");
    // (coef[4] == 0: the history is not read, only overwritten -- sched_step's noise check passes with the pointer set)
    return sched_step(sched_mode_word(RLDM_SAMPLER_DPMSOLVER, prediction_type), coef, model_output, x, x0_history, x_prev, n, stream);
}
int rldm_sched_unipc_step(int prediction_type, const float coef[12], const float* model_output, const float* x, float* last,
                          float* hist, float* x_prev, int64_t n, void* stream) {
    RLDM_REQUIRE(prediction_type >= RLDM_PRED_EPSILON && prediction_type <= RLDM_PRED_SAMPLE, "unknown prediction type");
    RLDM_REQUIRE(coef && model_output && x && last && hist && x_prev && n >= 1, "null argument");
    auto overlap = [](const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; };
    RLDM_REQUIRE(!overlap(last, n, hist, 3 * n), "last and hist must not overlap");
    for (const float* t : {model_output, x, static_cast<const float*>(x_prev)})
        RLDM_REQUIRE(!overlap(t, n, last, n) && !overlap(t, n, hist, 3 * n), "last / hist must not overlap another tensor");
    RLDM_REQUIRE(x_prev == x || !overlap(x_prev, n, x, n), "x_prev may be x itself, not a tensor that overlaps it in part");
    RLDM_REQUIRE(!overlap(x_prev, n, model_output, n), "x_prev must not overlap model_output");
    UniPCParams up;
    memset(&up, 0, sizeof(up));
    up.pred = prediction_type;
    for (int i = 0; i < 12; ++i) up.coef[i] = coef[i];
    up.out = model_output; up.x = x; up.last = last; up.hist = hist; up.x_prev = x_prev; up.n = n;
    return launch_sched_unipc_step(up, reinterpret_cast<hipStream_t>(stream));
}
int rldm_sched_step(int sampler_mode, int prediction_type, const float coef[5], const float* model_output, const float* x,
                    const float* noise, float* x_prev, int64_t n, void* stream) {
    RLDM_REQUIRE(sampler_mode == RLDM_SAMPLER_DDIM || sampler_mode == RLDM_SAMPLER_DDPM, "unknown sampler mode");
    RLDM_REQUIRE(prediction_type >= RLDM_PRED_EPSILON && prediction_type <= RLDM_PRED_SAMPLE, "unknown prediction type");
    return sched_step(sched_mode_word(sampler_mode, prediction_type), coef, model_output, x, noise, x_prev, n, stream);
}
int rldm_sched_guided_step(int sampler_mode, int prediction_type, const float coef[9], const float* model_output, const float* x,
                           const float* noise, const float* known, const float* mask, const float* known_noise,
                           const float* renoise_noise, float* x_prev, int B, int C, int64_t spatial, void* stream) {
    RLDM_REQUIRE(sampler_mode == RLDM_SAMPLER_DDIM || sampler_mode == RLDM_SAMPLER_DDPM, "guided step: sampler mode must be DDIM or DDPM");
    RLDM_REQUIRE(prediction_type >= RLDM_PRED_EPSILON && prediction_type <= RLDM_PRED_SAMPLE, "unknown prediction type");
    RLDM_REQUIRE(coef && model_output && x && known && mask && x_prev, "null argument");
    RLDM_REQUIRE(B >= 1 && C >= 1 && spatial >= 1, "guided step: empty shape");
    RLDM_REQUIRE(coef[4] == 0.f || noise != nullptr, "sigma != 0 requires a noise tensor");
    RLDM_REQUIRE(coef[6] == 0.f || known_noise != nullptr, "kb != 0 requires a known_noise tensor");
    RLDM_REQUIRE((coef[7] == 1.f && coef[8] == 0.f) || renoise_noise != nullptr, "(ra, rb) != (1, 0) requires a renoise_noise tensor");
    GuidedSchedParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.s.mode = (sampler_mode == RLDM_SAMPLER_DDIM ? 0 : 1) | (prediction_type << 1);
    for (int i = 0; i < 5; ++i) gp.s.coef[i] = coef[i];
    for (int i = 0; i < 4; ++i) gp.k[i] = coef[5 + i];
    gp.s.eps = model_output; gp.s.x = x; gp.s.noise = noise; gp.s.x_prev = x_prev;
    gp.known = known; gp.mask = mask; gp.known_noise = known_noise; gp.renoise_noise = renoise_noise;
    gp.spatial = spatial;
    gp.per_sample = spatial * C;
    gp.s.n = gp.per_sample * B;
    return launch_sched_guided_step(gp, reinterpret_cast<hipStream_t>(stream));
}
int rldm_sched_add_noise(const float* x0, const float* noise, const float* sqrt_alpha, const float* sqrt_beta, int B,
                         int64_t per_sample, float* out, void* stream) {
    RLDM_REQUIRE(x0 && noise && sqrt_alpha && sqrt_beta && out, "null argument");
    return launch_add_noise(x0, noise, sqrt_alpha, sqrt_beta, B, per_sample, out, reinterpret_cast<hipStream_t>(stream));
}

// ---- sampler ------------------------------------------------------------------------------------------------------
static int sampler_num_lanes(int batch, int W, int H) {
    // ONE chain up to batch 31: chains of fewer than 16 samples lose more to the fixed cost of every launch than they gain
    // from running side by side (batch 16: two chains of 8 measured 165 img/s against 194 for a single chain).  From batch
    // 32 on, chains of >= 16 samples overlap usefully (the launches of one chain fill the CUs the other leaves idle in its
    // prologues / low-resolution levels): 2 x 16 = 241 img/s against 229 for one chain of 32, 3 x 16 = 264 against 1 x 48,
    // 2 x 32 = 267 against 264 for one chain of 64; four chains were slower again (238).  RLDM_LANES=n overrides.
    // The unit is WORK, not samples: a chain wants >= 16 x 4096 network-input pixels (16 KITTI latents of 256 x 16).  nuScenes
    // latents are 256 x 8: 32 of them as 2 x 16 measured 301 img/s against 358 for one chain, so they split from 64 on.
    const long long px = (long long)batch * W * H, unit = 16LL * 4096;
    // Pixel-space networks (RangeDM, 1024 x 64 per sample) fill the chip with every launch of a single sample: 2 chains of 2
    // measured 91 img/s against 93.5 for one chain of 4, so only latent-space samplers split.
    int want = (px >= 2 * unit && W * H <= 8192) ? (int)std::min<long long>(3, px / unit) : 1;
    if (const char* e = getenv("RLDM_LANES")) want = atoi(e);
    if (want <= 0) want = 1;
    want = std::max(1, std::min(want, batch));
    while (batch % want) --want;
    return want;
}

int rldm_sampler_create(rldm_unet* unet, rldm_vae* vae, const rldm_sampler_config* cfg, rldm_sampler** out) {
    RLDM_REQUIRE(unet && cfg && out, "null argument");
    RLDM_REQUIRE(unet->params.finalized, "unet not finalized");
    RLDM_REQUIRE(!vae || vae->params.finalized, "vae not finalized");
    RLDM_REQUIRE(cfg->batch >= 1 && cfg->num_steps >= 1 && cfg->coef && cfg->timesteps, "bad sampler config");
    RLDM_REQUIRE(cfg->prediction_type >= RLDM_PRED_EPSILON && cfg->prediction_type <= RLDM_PRED_SAMPLE, "bad sampler config: prediction_type");
    RLDM_REQUIRE(cfg->mode == RLDM_SAMPLER_DDIM || cfg->mode == RLDM_SAMPLER_DDPM || cfg->mode == RLDM_SAMPLER_DPMSOLVER ||
                     cfg->mode == RLDM_SAMPLER_UNIPC, "bad sampler config: mode");
    RLDM_REQUIRE(cfg->guided == 0 || cfg->guided == 1, "bad sampler config: guided");
    RLDM_REQUIRE(!cfg->guided || (cfg->mode != RLDM_SAMPLER_DPMSOLVER && cfg->mode != RLDM_SAMPLER_UNIPC),
                 "a guided sampler runs DDIM (eta = 0) or DDPM rows: the x0 history of DPM-Solver++ and UniPC means nothing across a jump back up");
    RLDM_REQUIRE(!cfg->guided || cfg->cond_channels == 0, "a guided sampler is unconditional (cond_channels == 0)");
    const int coef_w = cfg->guided ? 9 : cfg->mode == RLDM_SAMPLER_UNIPC ? 12 : 5;
    if (cfg->guided)
        for (int i = 0; i < cfg->num_steps; ++i)
            RLDM_REQUIRE(cfg->mode != RLDM_SAMPLER_DDIM || cfg->coef[(size_t)i * 9 + 4] == 0.f, "a guided DDIM sampler needs eta = 0 rows");
    const auto& uc = unet->cfg;
    RLDM_REQUIRE(uc.out_channels + (cfg->pos_encoding ? 1 : 0) + cfg->cond_channels == uc.in_channels,
                 "unet.in_channels != out_channels + pos_encoding + cond_channels (ldm/pipelines.py:351,480)");
    RLDM_REQUIRE(!vae || vae->cfg.z_channels == uc.out_channels, "vae latent channels != unet out_channels");
    auto s = std::make_unique<rldm_sampler>();
    s->unet = unet;
    s->vae = vae;
    s->cfg = *cfg;
    s->cfg.coef = nullptr;
    s->cfg.timesteps = nullptr;
    s->plan_flags = cfg->plan_flags;
    RLDM_HIP_CHECK(hipGetDevice(&s->device));
    const int B = cfg->batch, W = uc.sample_w, H = uc.sample_h;
    const long long per_latent = (long long)uc.out_channels * W * H;
    const long long per_cond = (long long)cfg->cond_channels * W * H;
    long long per_image = 0;
    if (vae) {
        const int f = 1 << (vae->cfg.num_levels - 1);
        per_image = (long long)vae->cfg.out_channels * (W * f) * (H * f);
    }
    s->n_latent = B * per_latent;
    s->n_image = B * per_image;
    RLDM_HIP_CHECK(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
    if (upload(s->coef, cfg->coef, (size_t)cfg->num_steps * coef_w * 4)) return 1;
    if (cfg->guided)
        for (int i = 0; i < cfg->num_steps; ++i) {
            const float* r = cfg->coef + (size_t)i * 9;
            s->needs_known_noise |= r[6] != 0.f;
            s->needs_renoise_noise |= r[7] != 1.f || r[8] != 0.f;
        }
    std::vector<float> tf(cfg->num_steps);
    for (int i = 0; i < cfg->num_steps; ++i) tf[i] = (float)cfg->timesteps[i];
    if (upload(s->t_dev, tf.data(), tf.size() * 4)) return 1;
    const int nl = sampler_num_lanes(B, W, H);
    for (int l = 0; l < nl; ++l) {
        auto ln = std::make_unique<SamplerLane>();
        ln->nb = B / nl;
        ln->b0 = l * ln->nb;
        ln->n_latent = ln->nb * per_latent;
        ln->n_image = ln->nb * per_image;
        ln->n_cond = ln->nb * per_cond;
        RLDM_HIP_CHECK(hipStreamCreateWithFlags(&ln->stream, hipStreamNonBlocking));
        RLDM_HIP_CHECK(hipEventCreateWithFlags(&ln->ev_out, hipEventDisableTiming));
        if (ln->x.alloc(ln->n_latent * 4) || ln->eps.alloc(ln->n_latent * 4) || ln->step.alloc(64)) return 1;
        if (cfg->mode == RLDM_SAMPLER_DPMSOLVER && ln->hist.alloc(ln->n_latent * 4)) return 1;
        if (cfg->mode == RLDM_SAMPLER_UNIPC && (ln->hist.alloc(ln->n_latent * 3 * 4) || ln->last.alloc(ln->n_latent * 4))) return 1;
        if (cfg->cond_channels && ln->cond.alloc((size_t)ln->n_cond * 4)) return 1;
        if (vae && ln->image.alloc(ln->n_image * 4)) return 1;
        s->lanes.push_back(std::move(ln));
    }
    if (sampler_build_plans(s.get())) return 1;
    {
        std::lock_guard<std::mutex> lk(g_samplers_mu);
        g_samplers.push_back(s.get());
    }
    *out = s.release();
    return 0;
}
void rldm_sampler_destroy(rldm_sampler* s) { delete s; }

// this sampler's plans again, every layer a launch of its own (same kernels, same tiles: RLDM_FLAG_NO_PERSISTENT, scoped to it)
static int sampler_drop_persistent(rldm_sampler* s, const char* why, int code) {
    fprintf(stderr, "librangeldm_hip: %s (code %d); this sampler runs one launch per layer from here on\n", why, code);
    s->plan_flags |= RLDM_FLAG_NO_PERSISTENT;
    return sampler_build_plans(s);
}

// Self-check of the LAST rldm_sample call: waits for the call (the lanes' final events), then reads the word its persistent launches
// left.  0: the call's outputs are valid.  Non-zero (1 a cluster wait gave up, 2 a cluster was spread over several XCDs): the outputs
// were NaN-marked, rldm_last_error says why, and the sampler has already rebuilt itself without persistent launches -- call again.
int rldm_sampler_status(rldm_sampler* s) {
    RLDM_REQUIRE(s, "null argument");
    int code = 0;
    for (auto& lnp : s->lanes) {
        SamplerLane* ln = lnp.get();
        if (!ln->check_pending) continue;
        RLDM_HIP_CHECK(hipEventSynchronize(ln->ev_out));
        ln->check_pending = false;
        if (*ln->check_host != 0) code = *ln->check_host;
    }
    if (s->latched_error) { code = s->latched_error; s->latched_error = 0; }
    if (code == 0) return 0;
    if (sampler_drop_persistent(s, "a persistent launch of the last rldm_sample call failed its self-check", code)) return -1;
    set_error("a persistent launch of this rldm_sample call failed its self-check (code " + std::to_string(code) +
              ": 1 a cluster wait gave up -- the GPU was shared with other work --, 2 a cluster was spread over several XCDs); the call's "
              "outputs are invalid and NaN-marked; the sampler now runs one launch per layer: call rldm_sample again");
    return code;
}

int rldm_debug_inject_trunk_error(rldm_sampler* s, int code) {
    RLDM_REQUIRE(s, "null argument");
    s->inject_error = code;
    return 0;
}

// the previous call's persistent launches failed their self-check (its outputs were NaN-marked): rebuild without them, fail this call
// (the NO_PERSISTENT guard comes from the latched-error site; the pending-word site had none and needs none: a plan built under
//  that flag has no self-check word, so the word is never pending -- there the guard is always true)
static int previous_call_failed(rldm_sampler* s, int code) {
    if (!(s->plan_flags & RLDM_FLAG_NO_PERSISTENT) && sampler_drop_persistent(s, "a persistent launch of the PREVIOUS rldm_sample call failed its self-check", code)) return 1;
    RLDM_REQUIRE(false, "a persistent launch of the PREVIOUS rldm_sample call failed its self-check (code " + std::to_string(code) +
                            "): its outputs were invalid (NaN-marked); the sampler now runs one launch per layer: call again");
    return 1;
}

// the lane back at the head of the call's chain: x_T in x (the caller's, or purpose 0 / row 0 of the call's generator for the lane's
// samples), conv_in's input packed from it, the step word at its start
static int lane_rewind(rldm_sampler* s, SamplerLane* ln, const SampleCall& c, hipStream_t st) {
    if (c.x_T) {
        const size_t lat_off = (size_t)ln->b0 * (ln->n_latent / ln->nb);
        RLDM_HIP_CHECK(hipMemcpyAsync(ln->x.p, c.x_T + lat_off, ln->n_latent * 4, hipMemcpyDeviceToDevice, st));
    } else if (launch_rng_fill(lane_rng_fill(ln, ln->x.as<float>()), st)) {
        return 1;
    }
    if (sampler_pack_x(s, ln, st)) return 1;
    return launch_step_counter(ln->step.as<int>(), ln->fused_tail ? -1 : 0, 0, st);
}

static int sample_impl(rldm_sampler* s, const SampleCall& c) {
    RLDM_REQUIRE(s && (c.x_T || c.rng_on), "null argument");
    RLDM_REQUIRE(c.images || c.latents_out, "no output requested");
    RLDM_REQUIRE((s->cfg.cond_channels == 0) == (c.cond == nullptr), "cond tensor does not match sampler.cond_channels");
    RLDM_REQUIRE(s->cfg.mode != RLDM_SAMPLER_DDPM || c.step_noise != nullptr || c.rng_on, "DDPM sampling needs step_noise");
    hipStream_t caller = reinterpret_cast<hipStream_t>(c.stream);
    if (s->unet_gen != s->unet->generation || (s->vae && s->vae_gen != s->vae->generation) || !s->unet->params.finalized ||
        (s->vae && !s->vae->params.finalized)) {
        if (sampler_build_plans(s)) return 1;       // the models were reloaded since the graphs were captured
    }
    // a host that did not ask rldm_sampler_status about the previous call learns here that it failed (its outputs were NaN-marked);
    // the sampler has rebuilt itself without persistent launches by the time this returns, so the retry is valid
    for (auto& lnp : s->lanes) {
        SamplerLane* ln = lnp.get();
        if (ln->check_pending && hipEventQuery(ln->ev_out) == hipSuccess) {
            ln->check_pending = false;
            const int code = *ln->check_host;
            if (code != 0) return previous_call_failed(s, code);
        }
    }
    // persistent launches need the device to themselves: another sampler's call still in flight on a different stream ends them here
    if (s->has_persistent()) {
        bool shared = s->shared_mark.exchange(false);
        {
            std::lock_guard<std::mutex> lk(g_samplers_mu);
            for (rldm_sampler* o : g_samplers)
                if (o != s && o->device == s->device && o->last_caller.load() != caller && o->in_flight()) {
                    shared = true;
                    o->shared_mark.store(true);     // (the peer keeps its spin-waiting clusters for the call in flight; not for the next)
                }
        }
        if (shared && sampler_drop_persistent(s, "another sampler is running on this device on a different stream: persistent launches "
                                                 "need the chip to themselves", 0)) return 1;
    }
    if (s->latched_error) {                         // found while the plans were rebuilt (sampler_build_plans): the previous call failed
        const int code = s->latched_error;
        s->latched_error = 0;
        return previous_call_failed(s, code);
    }
    s->last_caller.store(caller);
    RLDM_HIP_CHECK(hipEventRecord(s->ev_in, caller));
    // per lane: inputs, (first call) eager warm step + graph capture
    for (auto& lnp : s->lanes) {
        SamplerLane* ln = lnp.get();
        hipStream_t st = ln->stream;
        const size_t lat_off = (size_t)ln->b0 * (ln->n_latent / ln->nb);
        RLDM_HIP_CHECK(hipStreamWaitEvent(st, s->ev_in, 0));
        if (c.rng_on) {
            // the call's generator, stream-ordered in front of everything that reads it (no host synchronisation)
            if (!ln->rng_record.p && ln->rng_record.alloc(64)) return 1;
            if (launch_rng_record(ln->rng_record.as<unsigned>(), c.rng_seed, c.rng_draw, c.rng_offset, st)) return 1;
            if (s->cfg.mode == RLDM_SAMPLER_DDPM && !ln->rng_step.p && ln->rng_step.alloc(ln->n_latent * 4)) return 1;
            if (s->needs_known_noise && !ln->rng_known.p && ln->rng_known.alloc(ln->n_latent * 4)) return 1;
            if (s->needs_renoise_noise && !ln->rng_renoise.p && ln->rng_renoise.alloc(ln->n_latent * 4)) return 1;
        }
        if (c.cond)
            RLDM_HIP_CHECK(hipMemcpyAsync(ln->cond.p, c.cond + (size_t)ln->b0 * (ln->n_cond / ln->nb), ln->n_cond * 4,
                                          hipMemcpyDeviceToDevice, st));
        if (lane_rewind(s, ln, c, st)) return 1;
        const float* noise = s->cfg.mode != RLDM_SAMPLER_DDPM ? nullptr : c.rng_on ? ln->rng_step.as<float>() : c.step_noise + lat_off;
        ln->guided = GuidedIO();
        if (s->cfg.guided) {                        // each offset to the lane's first sample, exactly as step_noise is
            ln->guided.known = c.gio.known + lat_off;
            ln->guided.mask = c.gio.mask + (size_t)ln->b0 * s->unet->cfg.sample_w * s->unet->cfg.sample_h;
            ln->guided.known_noise = c.gio.known_noise ? c.gio.known_noise + lat_off : nullptr;
            ln->guided.renoise_noise = c.gio.renoise_noise ? c.gio.renoise_noise + lat_off : nullptr;
            if (c.rng_on) {
                ln->guided.known_noise = s->needs_known_noise ? ln->rng_known.as<float>() : nullptr;
                ln->guided.renoise_noise = s->needs_renoise_noise ? ln->rng_renoise.as<float>() : nullptr;
            }
        }
        if (!ln->step_graph || ln->captured_noise != noise || !(ln->captured_guided == ln->guided)) {
            // one eager step first (sets kernel attributes, packs weights), then rewind and capture
            if (sampler_enqueue_step(s, ln, c, noise, st)) return 1;
            RLDM_HIP_CHECK(hipStreamSynchronize(st));
            if (ln->uplan->trunk_error.p) {         // the persistent trunk's self-check (a wait that gave up / a cluster off its XCD)
                int terr = 0;
                RLDM_HIP_CHECK(hipMemcpy(&terr, ln->uplan->trunk_error.p, 4, hipMemcpyDeviceToHost));
                const bool off = ((dbg_process() | s->plan_flags) & RLDM_FLAG_NO_PERSISTENT) != 0;
                if (getenv("RLDM_TEST_TRUNK_FAIL") && !off) terr = 2;      // (tests: the fall-back path below)
                if (terr != 0 && !off) {
                    // the clusters' only assumption (an image's workgroups share an XCD; all of them resident) does not hold on this
                    // device / driver / right now: THIS sampler runs every layer as a launch of its own from here on (same kernels, tiles)
                    if (sampler_drop_persistent(s, "persistent launches failed their self-check at the warm-up step", terr)) return 1;
                    return sample_impl(s, c);
                }
                RLDM_REQUIRE(terr == 0, "persistent trunk launch failed its self-check (code " + std::to_string(terr) +
                                            "): set RLDM_DBG_FLAGS=16777216 to run the levels as separate launches");
            }
            if (lane_rewind(s, ln, c, st)) return 1;
            // the graph holds `gs` consecutive steps (the step index lives on the device, so the steps are identical launches):
            // fewer, longer graphs keep the queue fed across step boundaries
            int gs = std::max(1, std::min(kGraphSteps, s->cfg.num_steps));
            while (s->cfg.num_steps % gs != 0) --gs;
            ln->graph_steps = gs;
            if (capture(st, [&]() {
                    for (int k = 0; k < gs; ++k)
                        if (sampler_enqueue_step(s, ln, c, noise, st)) return 1;
                    return 0;
                }, &ln->step_graph)) return 1;
            ln->captured_noise = noise;
            ln->captured_guided = ln->guided;
            ++s->captures;
        }
        if (c.images && s->vae && !ln->decode_graph) {
            // (the decode runs on whatever x holds now: only its launch list is recorded)
            if (ln->dplan->run(st)) return 1;
            RLDM_HIP_CHECK(hipStreamSynchronize(st));
            if (capture(st, [&]() { return ln->dplan->run(st); }, &ln->decode_graph)) return 1;
            if (lane_rewind(s, ln, c, st)) return 1;         // (also rewrites the step word with the value it holds: one launch, first call only)
        }
    }
    if (s->inject_error) {                          // tests: a cluster wait that gave up in the middle of a run
        for (auto& lnp : s->lanes)
            if (lnp->uplan->trunk_error.p && launch_step_counter(lnp->uplan->trunk_error.as<int>(), s->inject_error, 0, lnp->stream)) return 1;
        s->inject_error = 0;
    }
    // the chains: step-major so every stream always has work queued
    for (int i = 0; i < s->cfg.num_steps; i += s->lanes[0]->graph_steps)
        for (auto& lnp : s->lanes) RLDM_HIP_CHECK(hipGraphLaunch(lnp->step_graph, lnp->stream));
    for (auto& lnp : s->lanes) {
        SamplerLane* ln = lnp.get();
        hipStream_t st = ln->stream;
        const size_t lat_off = (size_t)ln->b0 * (ln->n_latent / ln->nb);
        if (c.latents_out)
            RLDM_HIP_CHECK(hipMemcpyAsync(c.latents_out + lat_off, ln->x.p, ln->n_latent * 4, hipMemcpyDeviceToDevice, st));
        if (c.images) {
            if (s->vae) {
                RLDM_HIP_CHECK(hipGraphLaunch(ln->decode_graph, st));
                RLDM_HIP_CHECK(hipMemcpyAsync(c.images + (size_t)ln->b0 * (ln->n_image / ln->nb), ln->image.p, ln->n_image * 4,
                                              hipMemcpyDeviceToDevice, st));
            } else {
                RLDM_HIP_CHECK(hipMemcpyAsync(c.images + lat_off, ln->x.p, ln->n_latent * 4, hipMemcpyDeviceToDevice, st));
            }
        }
        if (ln->uplan->trunk_error.p) {
            // same-call failure signal: the call's outputs are NaN-marked on the device if a persistent launch gave up a wait, and
            // the word travels to pinned memory for rldm_sampler_status (no host synchronisation here)
            if (!ln->check_host) {
                RLDM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ln->check_host), 64, hipHostMallocDefault));
                *ln->check_host = 0;
            }
            float* img_l = c.images ? c.images + (s->vae ? (size_t)ln->b0 * (ln->n_image / ln->nb) : lat_off) : nullptr;
            if (launch_trunk_check(ln->uplan->trunk_error.as<int>(), img_l, s->vae ? ln->n_image : ln->n_latent,
                                   c.latents_out ? c.latents_out + lat_off : nullptr, ln->n_latent, st)) return 1;
            RLDM_HIP_CHECK(hipMemcpyAsync(ln->check_host, ln->uplan->trunk_error.p, 4, hipMemcpyDeviceToHost, st));
            ln->check_pending = true;
        }
        RLDM_HIP_CHECK(hipEventRecord(ln->ev_out, st));
        ln->call_recorded = true;
        RLDM_HIP_CHECK(hipStreamWaitEvent(caller, ln->ev_out, 0));
    }
    return 0;
}

int rldm_sample(rldm_sampler* s, const float* x_T, const float* step_noise, const float* cond, float* images,
                float* latents_out, void* stream) {
    RLDM_REQUIRE(s, "null argument");
    RLDM_REQUIRE(!s->cfg.guided, "this sampler was created with guided = 1: call rldm_sample_guided (known, mask and the two noise "
                                 "tensors are part of every row)");
    SampleCall c;
    c.x_T = x_T; c.step_noise = step_noise; c.cond = cond;
    c.images = images; c.latents_out = latents_out; c.stream = stream;
    return sample_impl(s, c);
}

int rldm_sample_guided(rldm_sampler* s, const float* x_T, const float* step_noise, const float* known, const float* mask,
                       const float* known_noise, const float* renoise_noise, float* images, float* latents_out, void* stream) {
    RLDM_REQUIRE(s, "null argument");
    RLDM_REQUIRE(s->cfg.guided, "rldm_sample_guided needs a sampler created with guided = 1");
    RLDM_REQUIRE(known && mask, "null argument: known / mask");
    RLDM_REQUIRE(known_noise || !s->needs_known_noise, "some row has kb != 0: known_noise must be given");
    RLDM_REQUIRE(renoise_noise || !s->needs_renoise_noise, "some row jumps back up: renoise_noise must be given");
    SampleCall c;
    c.x_T = x_T; c.step_noise = step_noise;
    c.gio.known = known; c.gio.mask = mask; c.gio.known_noise = known_noise; c.gio.renoise_noise = renoise_noise;
    c.images = images; c.latents_out = latents_out; c.stream = stream;
    return sample_impl(s, c);
}

// the two calls above with the noise drawn inside the step graph (rng.hip): the generator in place of the noise tensors
static int sampler_set_generator(const rldm_sampler* s, uint64_t seed, uint32_t draw, uint64_t sample_offset, SampleCall* c) {
    RLDM_REQUIRE(draw < (1u << 30), "draw must be below 2^30 (stream = 4 * draw + purpose is 32 bits)");
    RLDM_REQUIRE(sample_offset + (uint64_t)s->cfg.batch <= (1ULL << 32), "sample_offset + batch must not exceed 2^32");
    RLDM_REQUIRE(s->n_latent / s->cfg.batch < (1LL << 31), "a sample must hold fewer than 2^31 elements");
    c->rng_on = true;
    c->rng_seed = seed;
    c->rng_draw = draw;
    c->rng_offset = (uint32_t)sample_offset;
    return 0;
}

int rldm_sample_rng(rldm_sampler* s, const float* x_T, uint64_t seed, uint32_t draw, uint64_t sample_offset, const float* cond,
                    float* images, float* latents_out, void* stream) {
    RLDM_REQUIRE(s, "null argument");
    RLDM_REQUIRE(!s->cfg.guided, "this sampler was created with guided = 1: call rldm_sample_guided_rng");
    SampleCall c;
    if (sampler_set_generator(s, seed, draw, sample_offset, &c)) return 1;
    c.x_T = x_T; c.cond = cond;
    c.images = images; c.latents_out = latents_out; c.stream = stream;
    return sample_impl(s, c);
}

int rldm_sample_guided_rng(rldm_sampler* s, const float* x_T, uint64_t seed, uint32_t draw, uint64_t sample_offset, const float* known,
                           const float* mask, float* images, float* latents_out, void* stream) {
    RLDM_REQUIRE(s, "null argument");
    RLDM_REQUIRE(s->cfg.guided, "rldm_sample_guided_rng needs a sampler created with guided = 1");
    RLDM_REQUIRE(known && mask, "null argument: known / mask");
    SampleCall c;
    if (sampler_set_generator(s, seed, draw, sample_offset, &c)) return 1;
    c.x_T = x_T;
    c.gio.known = known; c.gio.mask = mask;
    c.images = images; c.latents_out = latents_out; c.stream = stream;
    return sample_impl(s, c);
}

int rldm_debug_sampler_captures(rldm_sampler* s) {
    RLDM_REQUIRE(s, "null argument");
    return s->captures;
}

// one instrumented UNet step + scheduler step (+ VAE decode) of lane 0: per-kernel launch counts, HIP-event time,
// algorithmic work.  JSON also carries "lanes" and "lane_batch" so the caller can scale to the whole batch.
int rldm_sampler_profile(rldm_sampler* s, const float* x_T, char* json_out, size_t cap) {
    RLDM_REQUIRE(s && x_T && json_out && cap > 2, "null argument");
    SamplerLane* ln = s->lanes[0].get();
    hipStream_t st = ln->stream;
    SampleCall c;
    c.x_T = x_T;
    if (lane_rewind(s, ln, c, st)) return 1;
    if (ln->uplan->run(st)) return 1;                      // warm
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    std::map<std::string, KernelStat> unet_stats, vae_stats;
    if (ln->uplan->run_profiled(st, unet_stats)) return 1;
    if (ln->dplan) {
        if (ln->dplan->run(st)) return 1;
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        if (ln->dplan->run_profiled(st, vae_stats)) return 1;
    }
    std::string js = "{";
    auto dump = [&](const char* key, const std::map<std::string, KernelStat>& m) {
        js += std::string("\"") + key + "\": {";
        bool first = true;
        for (auto& kv : m) {
            if (!first) js += ", ";
            first = false;
            char buf[512];
            snprintf(buf, sizeof(buf), "\"%s\": {\"launches\": %d, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}",
                     kv.first.c_str(), kv.second.launches, kv.second.ms, kv.second.flops, kv.second.bytes);
            js += buf;
        }
        js += "}";
    };
    dump("unet_step", unet_stats);
    js += ", ";
    dump("vae_decode", vae_stats);
    // routing bits in effect (rldm_sampler_config::plan_flags | the library's own fall-backs) and whether a fall-back engaged
    js += ", \"plan_flags\": " + std::to_string(s->plan_flags) + ", \"fell_back\": " + (s->plan_flags != s->cfg.plan_flags ? "true" : "false");
    js += ", \"lanes\": " + std::to_string(s->lanes.size()) + ", \"lane_batch\": " + std::to_string(ln->nb) + "}";
    RLDM_REQUIRE(js.size() + 1 <= cap, "profile buffer too small");
    memcpy(json_out, js.c_str(), js.size() + 1);
    return 0;
}

// timeline of the UNet ops inside the sampler's captured step graph (flag 8192 at sampler creation): stamps[i] =
// 100 MHz counter before op i (stamps[n] after the last), names = op kernel names joined by '\n'.  Returns the op count.
int rldm_debug_graph_trace(unsigned long long* stamps, int cap, char* names, size_t names_cap) {
    if (!g_trace.p || !g_trace_plan) return 0;
    (void)hipDeviceSynchronize();
    int n = 0;                                  // (the ops that launched: run_stamped leaves no stamp for the others)
    for (auto& o : g_trace_plan->ops) n += (!o.active || o.active()) ? 1 : 0;
    const int m = std::min(cap, n + 1);
    if (stamps && m > 0 && hipMemcpy(stamps, g_trace.p, (size_t)m * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (names && names_cap) {
        std::string all;
        for (auto& o : g_trace_plan->ops)
            if (!o.active || o.active()) all += o.name + "\n";
        strncpy(names, all.c_str(), names_cap - 1);
        names[names_cap - 1] = 0;
    }
    return n;
}

}  // extern "C"
