/*
 * rangeldm_hip.h -- C ABI of librangeldm_hip.so: the MI355X (gfx950) implementation of the RangeLDM denoising
 * hot path (UNet2DModel forward, DDPM/DDIM scheduler step, AutoencoderKL encode/decode, whole sampling loop).
 *
 * The reference has no FFI: the path sits behind Python duck-typing.  Each entry point below names
 * the reference call it replaces (file:line under the reference tree).  The python modules under rangeldm_amd/ are the thin ctypes shim
 * that re-presents these as `unet(x, t).sample`, `scheduler.step(...).prev_sample`, `vae.decode(z).sample` and
 * `pipe(batch_size=..., num_inference_steps=...)`; INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Conventions
 *   - Every function returns 0 on success, non-zero on failure; the message is in rldm_last_error() (thread-local).
 *     Nothing throws across the ABI.
 *   - Tensors at the boundary are the reference's: fp32, NCHW with dim2 = W (azimuth), dim3 = H (beams)
 *     (ldm/dataset.py:228-233), contiguous, resident in device (HBM) memory, owned by the caller.  Internally
 *     activations are bf16 channels-last [B][W][H][C] with fp32 accumulation; weights are owned by the library.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all work is enqueued on it (the
 *     sampler uses an internal stream fenced by events against `stream`).  Single caller thread per handle.
 */
#ifndef RANGELDM_HIP_H
#define RANGELDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLDM_MAX_LEVELS 8

typedef struct rldm_unet rldm_unet;       /* UNet2DModel replacement   */
typedef struct rldm_vae rldm_vae;         /* AutoencoderKL replacement */
typedef struct rldm_sampler rldm_sampler; /* Pipeline.__call__ loop    */

/* UNet2DModel(**model_config): ldm/train_unconditional.py:237-242, ldm/configs/RangeLDM.yaml:17-24.
 * Library defaults the reference relies on are explicit fields. */
typedef struct rldm_unet_config {
    int32_t sample_w, sample_h;                 /* sample_size = (W, H)                                  */
    int32_t in_channels, out_channels;
    int32_t layers_per_block;
    int32_t num_levels;
    int32_t block_out_channels[RLDM_MAX_LEVELS];
    int32_t down_attn[RLDM_MAX_LEVELS];         /* 1: AttnDownBlock2D, 0: DownBlock2D                    */
    int32_t up_attn[RLDM_MAX_LEVELS];           /* 1: AttnUpBlock2D,   0: UpBlock2D                      */
    int32_t attention_head_dim;                 /* 8 (only value supported by the d=8 attention kernel)  */
    int32_t norm_num_groups;                    /* 32                                                    */
    float norm_eps;                             /* 1e-5                                                  */
    int32_t mid_attention;                      /* add_attention                                         */
    int32_t flip_sin_to_cos;                    /* Timesteps(..., flip_sin_to_cos): 1 for UNet2DModel    */
    int32_t freq_shift;                         /* Timesteps(..., downscale_freq_shift): 0; (0, 1) is the
                                                   sinusoid of vae/sgm/modules/diffusionmodules/model.py:28-46 */
} rldm_unet_config;

/* sgm Encoder/Decoder kwargs: vae/configs/kitti360.yaml:30-62 (== AutoencoderKL after ldm/convert_vae.py:123-189). */
typedef struct rldm_vae_config {
    int32_t in_channels, out_channels;
    int32_t ch;
    int32_t num_levels;
    int32_t ch_mult[RLDM_MAX_LEVELS];
    int32_t num_res_blocks;
    int32_t z_channels;
    int32_t double_z;
    int32_t norm_num_groups;
    float norm_eps;                             /* 1e-6 */
    float scaling_factor;                       /* 0.18215, ldm/convert_vae.py:159-168 */
} rldm_vae_config;

const char* rldm_last_error(void);
/* 0 if a gfx950 device is usable; fills name (may be NULL). */
int rldm_device_info(char* name, size_t name_len, int* compute_units);

/* ---- UNet2DModel ------------------------------------------------------------------------------------------- */
/* replaces UNet2DModel(**cfg) + replace_down/replace_conv surgery: ldm/inference.py:84-85,102-104 */
int rldm_unet_create(const rldm_unet_config* cfg, rldm_unet** out);
void rldm_unet_destroy(rldm_unet* m);
/* replaces load_state_dict / safetensors.load_model (ldm/inference.py:120): one call per diffusers key,
 * `data` = HOST fp32, `numel` elements in the reference's (C_out, C_in, kh, kw) / (out, in) order. */
int rldm_unet_set_param(rldm_unet* m, const char* name, const float* data, int64_t numel);
/* checks every key was supplied, packs bf16 MFMA-ordered weights to HBM.  May be called again after further
 * rldm_unet_set_param calls (load_state_dict on a live model, e.g. periodic EMA evaluation): it frees and rebuilds the
 * device weights and bumps the model's generation; every rldm_sampler built on the model notices at its next
 * rldm_sample and re-plans / re-captures its graphs (between set_param and finalize the model refuses to run). */
int rldm_unet_finalize(rldm_unet* m);
/* replaces `unet(sample, timestep).sample` (ldm/pipelines.py:103,239,360,500; train: ldm/train_unconditional.py:512).
 * sample: device fp32 [B, in_channels, W, H]; timesteps: HOST int64, nt == 1 (broadcast) or nt == B;
 * out: device fp32 [B, out_channels, W, H]. */
int rldm_unet_forward(rldm_unet* m, const float* sample, const int64_t* timesteps, int nt, int B, float* out,
                      void* stream);

/* ---- AutoencoderKL ------------------------------------------------------------------------------------------ */
int rldm_vae_create(const rldm_vae_config* cfg, rldm_vae** out);     /* ldm/inference.py:86-96 */
void rldm_vae_destroy(rldm_vae* m);
int rldm_vae_set_param(rldm_vae* m, const char* name, const float* data, int64_t numel);  /* ldm/inference.py:97 */
int rldm_vae_finalize(rldm_vae* m);
/* replaces `vae.decode(z).sample` (ldm/pipelines.py:367,507).  z: device fp32 [B, z_channels, W/f, H/f] (already
 * divided by scaling_factor by the caller, as the reference does at :365); image: device fp32 [B, out_ch, W, H]. */
int rldm_vae_decode(rldm_vae* m, const float* z, int B, int latent_w, int latent_h, float* image, void* stream);
/* replaces `vae.encode(x)` up to the moments (ldm/train_unconditional.py:480, ldm/pipelines.py:408).
 * x: device fp32 [B, in_ch, W, H]; moments: device fp32 [B, 2*z, W/f, H/f] = [mean | logvar]. */
int rldm_vae_encode(rldm_vae* m, const float* x, int B, int w, int h, float* moments, void* stream);
/* replaces DiagonalGaussianDistribution.sample (vae/sgm/modules/distributions/distributions.py:24-41):
 * out = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale.  All device fp32; n = B*z*w*h elements of `out`. */
int rldm_diag_gaussian_sample(const float* moments, const float* noise, float scale, int B, int z, int spatial,
                              float* out, void* stream);

/* ---- scheduler steps (elementwise; coefficients computed by the host shim exactly as diffusers does) -------- */
/* replaces DDIMScheduler.step (ldm/pipelines.py:244-246), SURVEY.md B.2:
 *   x0 = (x - sqrt_beta_t*eps)/sqrt_alpha_t ; prev = sqrt_alpha_prev*x0 + dir_coef*eps + sigma*noise
 * coef = {sqrt_alpha_t, sqrt_beta_t, sqrt_alpha_prev, dir_coef, sigma}; noise may be NULL when sigma == 0. */
int rldm_sched_ddim_step(const float coef[5], const float* eps, const float* x, const float* noise, float* x_prev,
                         int64_t n, void* stream);
/* replaces DDPMScheduler.step (ldm/pipelines.py:106,362), SURVEY.md B.3:
 *   x0 = (x - sqrt_beta_t*eps)/sqrt_alpha_t ; prev = c_x0*x0 + c_xt*x + sigma*noise
 * coef = {sqrt_alpha_t, sqrt_beta_t, c_x0, c_xt, sigma}. */
int rldm_sched_ddpm_step(const float coef[5], const float* eps, const float* x, const float* noise, float* x_prev,
                         int64_t n, void* stream);
/* The same two steps for any `prediction_type` of the scheduler config (ldm/train_unconditional.py:345-352 passes it through;
 * :505-510 trains epsilon or v_prediction): what the network output means --
 *   RLDM_PRED_EPSILON  x0 = (x - sqrt_beta_t*out)/sqrt_alpha_t,      eps = out                 (the two entry points above)
 *   RLDM_PRED_V        x0 = sqrt_alpha_t*x - sqrt_beta_t*out,        eps = sqrt_alpha_t*out + sqrt_beta_t*x
 *   RLDM_PRED_SAMPLE   x0 = out,                                     eps = (x - sqrt_alpha_t*out)/sqrt_beta_t
 * then DDIM: prev = coef[2]*x0 + coef[3]*eps + coef[4]*noise; DDPM: prev = coef[2]*x0 + coef[3]*x + coef[4]*noise (coef as above).
 * sampler_mode: RLDM_SAMPLER_DDIM | RLDM_SAMPLER_DDPM. */
#define RLDM_PRED_EPSILON 0
#define RLDM_PRED_V 1
#define RLDM_PRED_SAMPLE 2
int rldm_sched_step(int sampler_mode, int prediction_type, const float coef[5], const float* model_output, const float* x,
                    const float* noise, float* x_prev, int64_t n, void* stream);
/* Guided (RePaint-style) step on an UNCONDITIONAL model: rldm_sched_step, then known-region replacement, then an optional
 * re-noise, one launch, fp32:
 *   u  = the step of rldm_sched_step(sampler_mode, prediction_type, coef[0..4], ...)      (the same expression, bit for bit)
 *   g  = m * (ka * z0 + kb * nk) + (1 - m) * u        z0 = `known`, nk = `known_noise`, m = `mask` (1: known)
 *   x' = ra * g + rb * nr                             nr = `renoise_noise`
 * coef = {the 5 of rldm_sched_step, ka, kb, ra, rb}: (ka, kb) = (sqrt(alpha_prod_prev), sqrt(1 - alpha_prod_prev)) of the row (1, 0
 * after the last timestep); (ra, rb) = (1, 0), or (sqrt(a_hi / a_lo), sqrt(1 - a_hi / a_lo)) on a row that jumps back up from
 * alpha_prod a_lo to a_hi (the forward noising across the levels in closed form, one draw).
 * model_output, x, noise, known, known_noise, renoise_noise, x_prev: device fp32 [B, C, spatial]; mask: device fp32 [B, 1, spatial],
 * broadcast over C.  m == 1 / m == 0 select: a known pixel does not depend on u (nor on a non-finite model output), an unknown one not
 * on z0.  ka * z0 + kb * nk is evaluated without contraction (bit-equal to the fp32 expression on a host).  known_noise is read only
 * when kb != 0, renoise_noise only when (ra, rb) != (1, 0), noise only when coef[4] != 0: each may be NULL otherwise.  x_prev may
 * alias x. */
int rldm_sched_guided_step(int sampler_mode, int prediction_type, const float coef[9], const float* model_output, const float* x,
                           const float* noise, const float* known, const float* mask, const float* known_noise,
                           const float* renoise_noise, float* x_prev, int B, int C, int64_t spatial, void* stream);
/* replaces DPMSolverMultistepScheduler.step (diffusers; algorithm_type "dpmsolver++", solver_type "midpoint", order 1 or 2,
 * final_sigmas_type "zero"): deterministic DPM-Solver++(2M).  Step i of N, sigma_i = sqrt((1-alpha_prod_t)/alpha_prod_t),
 * alpha_i = 1/sqrt(sigma_i^2+1), s_i = sigma_i*alpha_i, lambda_i = log alpha_i - log s_i (sigma_N = 0, lambda_N = +inf):
 *   x0 = the RLDM_PRED_* conversion above with sqrt_alpha_t = alpha_i, sqrt_beta_t = s_i
 *   prev = coef[2]*x0 + coef[3]*x + coef[4]*x0_prev
 * coef = {alpha_i, s_i, c_x0, c_xt, c_x0prev}; with h = lambda_{i+1} - lambda_i, phi = exp(-h) - 1 (-1 at the last step):
 *   first order (i == 0, solver_order 1, the last step):  c_x0 = -alpha_{i+1}*phi, c_xt = s_{i+1}/s_i, c_x0prev = 0
 *   second order, r = (lambda_i - lambda_{i-1})/h:        c_x0 = -alpha_{i+1}*phi*(1 + 1/(2r)), c_xt = s_{i+1}/s_i,
 *                                                         c_x0prev = alpha_{i+1}*phi/(2r)
 *   the last row is {alpha, s, 1, 0, 0}: the step returns x0.
 * x0_history: device fp32 [n], read only when coef[4] != 0 (it holds the previous step's x0), then overwritten with this
 * step's x0; it must not alias the other tensors.  The same rows are rldm_sampler_config::coef for RLDM_SAMPLER_DPMSOLVER. */
int rldm_sched_dpmsolver_step(int prediction_type, const float coef[5], const float* model_output, const float* x,
                              float* x0_history, float* x_prev, int64_t n, void* stream);
/* replaces UniPCMultistepScheduler.step (diffusers; solver_type "bh2", predict_x0, solver_order 1..3, lower_order_final,
 * final_sigmas_type "zero"): the predictor UniP and the corrector UniC of Zhao et al. 2023 on the grid of rldm_sched_dpmsolver_step.
 * Step i runs with order o_i = min(solver_order, N - i, steps taken + 1); m_k is the x0 prediction of step k.  One launch, fp32:
 *   m_i    = the RLDM_PRED_* conversion above with sqrt_alpha_t = alpha_i, sqrt_beta_t = s_i, on the x the network saw
 *   x_c    = use_corr ? k_last*last + k_1*m_{i-1} + k_2*m_{i-2} + k_3*m_{i-3} + k_t*m_i : x        (UniC of order o_{i-1}; i >= 1)
 *   x_prev = p_x*x_c + p_0*m_i + p_1*m_{i-1} + p_2*m_{i-2}                                        (UniP of order o_i)
 *   last <- x_c;  hist[2] <- hist[1];  hist[1] <- hist[0];  hist[0] <- m_i
 * coef = {alpha_i, s_i, use_corr, k_last, k_1, k_2, k_3, k_t, p_x, p_0, p_1, p_2}, from the host in float64
 * (rangeldm_amd/schedulers.py, UniPCMultistepSchedulerHIP: B = phi1 = expm1(-h), the rho of the R rho = b systems folded in); the last
 * row is {alpha, s, ., ..., 0, 1, 0, 0}: the step returns m_i.
 * last: device fp32 [n], the previous step's x_c; hist: device fp32 [3][n], hist[k] = m_{i-1-k} on entry.  Both are read only under a
 * non-zero coefficient (a term whose coefficient is 0 is left out, so a first step may find anything there, NaN included; the shift
 * still moves hist[0] and hist[1]) and rewritten element-wise by the thread that read them, so a replayed graph needs no pointer
 * rotation.  x_prev may be x itself (no other overlap with x, none with model_output).  last and hist must not overlap
 * model_output, x, x_prev or each other.  Any other overlap is refused.
 * The same rows are rldm_sampler_config::coef for RLDM_SAMPLER_UNIPC. */
int rldm_sched_unipc_step(int prediction_type, const float coef[12], const float* model_output, const float* x, float* last,
                          float* hist, float* x_prev, int64_t n, void* stream);
/* replaces DDPMScheduler.add_noise (ldm/train_unconditional.py:498): out = sa[b]*x0 + sb[b]*noise (sa, sb HOST [B]).
 * DDPMScheduler.get_velocity (ldm/train_unconditional.py:508) is the same map: v = sa[b]*noise - sb[b]*x0, i.e. this entry point
 * with (x0, noise) swapped and sb negated (rangeldm_amd/schedulers.py get_velocity). */
int rldm_sched_add_noise(const float* x0, const float* noise, const float* sqrt_alpha, const float* sqrt_beta, int B,
                         int64_t per_sample, float* out, void* stream);

/* ---- whole sampling loop (HIP-graph captured) --------------------------------------------------------------- */
#define RLDM_SAMPLER_DDIM 0   /* eta = 0 DDIM  (DDIMPipelineRange, ldm/pipelines.py:144-258; BASELINE metric) */
#define RLDM_SAMPLER_DDPM 1   /* strided ancestral DDPM (LDMPipelineRange as shipped, ldm/pipelines.py:282-383) */
#define RLDM_SAMPLER_DPMSOLVER 2   /* DPM-Solver++(2M), rows of rldm_sched_dpmsolver_step; each lane keeps its x0 history on the
                                    * device, so rldm_sample takes no step_noise (NULL) and no state carries between calls */
#define RLDM_SAMPLER_UNIPC 3       /* UniPC (bh2), rows of rldm_sched_unipc_step; each lane keeps `last` and the three-entry x0 history
                                    * on the device; unguided only, no step_noise, no state carries between calls.  The step is always
                                    * a launch of its own behind conv_out (as with RLDM_FLAG_SCHED_LAUNCH) */

typedef struct rldm_sampler_config {
    int32_t batch;            /* per-GPU batch                                                                */
    int32_t num_steps;        /* num_inference_steps                                                          */
    int32_t mode;             /* RLDM_SAMPLER_*                                                               */
    int32_t pos_encoding;     /* extra constant channel: 1 at azimuth 0 (ldm/pipelines.py:229-232,346-349)     */
    int32_t cond_channels;    /* channels of the per-step concatenated condition (ldm/pipelines.py:498), or 0  */
    /* 1: a guided sampler (rldm_sample_guided).  num_steps = the ROWS of its program, timesteps[row] may repeat and go back up,
     * coef = [rows][9] in the layout of rldm_sched_guided_step.  RLDM_SAMPLER_DDIM (eta = 0) or RLDM_SAMPLER_DDPM only.  The scheduler
     * step of such a sampler is always a launch of its own (as with RLDM_FLAG_SCHED_LAUNCH): the blend comes after it, so conv_out's
     * epilogue cannot pack the next step's input.  0 (what a zeroed struct says): everything else here, unchanged.  The field is the
     * newest one; it sits in what was the alignment hole in front of `coef`, so no existing offset and not the struct's size moved. */
    int32_t guided;
    /* per-step scheduler coefficients, HOST, [num_steps][5] in the layout of rldm_sched_{ddim,ddpm,dpmsolver}_step ([9]: guided;
     * [12]: RLDM_SAMPLER_UNIPC, the layout of rldm_sched_unipc_step) */
    const float* coef;
    /* timesteps, HOST int64 [num_steps] (scheduler.timesteps)                                                 */
    const int64_t* timesteps;
    /* routing options of THIS sampler's plans: RLDM_FLAG_* bits (enum rldm_flag), scoped to the sampler (0: defaults).
     * RLDM_FLAG_NO_PERSISTENT = every layer a launch of its own -- what a host sets for a sampler it knows will share the GPU. */
    int32_t plan_flags;
    /* RLDM_PRED_*: what the UNet's output means to the scheduler step (scheduler.config.prediction_type)               */
    int32_t prediction_type;
} rldm_sampler_config;

/* replaces Pipeline.__init__ + the per-call setup of ldm/pipelines.py:329-349; vae may be NULL (pixel-space RangeDM) */
int rldm_sampler_create(rldm_unet* unet, rldm_vae* vae, const rldm_sampler_config* cfg, rldm_sampler** out);
void rldm_sampler_destroy(rldm_sampler* s);
/* replaces the loop + decode of ldm/pipelines.py:353-367 (:496-507 with cond, :234-246 without VAE).
 * x_T: device fp32 [B, out_ch, W, H]; step_noise: device fp32 [num_steps, B, out_ch, W, H] (DDPM) or NULL (DDIM, DPMSOLVER, UNIPC);
 * cond: device fp32 [B, cond_channels, W, H] or NULL; images: device fp32 [B, 2, 4W, 4H] (or the final x_0 when
 * the sampler has no VAE); latents_out: optional device fp32 [B, out_ch, W, H] receiving the final latent. */
int rldm_sample(rldm_sampler* s, const float* x_T, const float* step_noise, const float* cond, float* images,
                float* latents_out, void* stream);
/* rldm_sample for a sampler created with guided = 1: every row runs the UNet, then rldm_sched_guided_step with the row's coefficients.
 * known: device fp32 [B, out_ch, W, H] (the clean known sample z0, at the UNet's sample resolution); mask: device fp32 [B, 1, W, H];
 * known_noise / renoise_noise: device fp32 [rows, B, out_ch, W, H], each NULL when every row's coefficient for it is zero (kb; rb).
 * step_noise: [rows, B, out_ch, W, H] (DDPM) or NULL (DDIM).  No cond.  rldm_sample refuses a guided sampler and this call an
 * unguided one; rldm_sampler_status covers both. */
int rldm_sample_guided(rldm_sampler* s, const float* x_T, const float* step_noise, const float* known, const float* mask,
                       const float* known_noise, const float* renoise_noise, float* images, float* latents_out, void* stream);
/* The reference's contract is "a correct tensor or an exception" (ldm/pipelines.py:218-222,463-464).  rldm_sample is asynchronous,
 * so the exception half is this call: it waits for the last rldm_sample of `s` and returns 0 when its outputs are valid.  Non-zero
 * = the self-check of the call's persistent launches tripped (1: a wait inside a workgroup cluster gave up, i.e. the GPU was shared
 * with other work; 2: a cluster was spread over several XCDs); the outputs of that call were NaN-marked ON THE DEVICE by the call's
 * last launch (so an unchecked consumer cannot mistake them for images), rldm_last_error() explains, and the sampler has already
 * rebuilt its plans as one launch per layer: calling rldm_sample again gives valid images.  The Python shim calls it in every
 * pipeline __call__ and raises RuntimeError. */
int rldm_sampler_status(rldm_sampler* s);

/* ---- counter-based normals (rangeldm_amd/csrc/rng.hip; the numpy statement is rangeldm_amd/rng.py) ------------------------
 * normal(seed, stream, row, sample, e): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (e >> 2, sample, row,
 * stream), whose words (o0, o1, o2, o3) give four normals by two Box-Muller pairs; element e takes z[e & 3].  stream = 4 * draw +
 * purpose (0 x_T and any plain randn, row 0; 1 step noise, 2 known-region noise, 3 re-noise of row r).  Known answers of the block:
 *   counter 0, key 0                         -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   counter 0xffffffff x 4, key 0xffffffff x 2 -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 * rldm_randn: out device fp32 [B][per_sample] = normal(seed, stream, row, sample_offset + b, e).  per_sample < 2^31 and
 * sample_offset + B <= 2^32, so the values of a sample do not depend on B or on how a batch is cut. */
int rldm_randn(float* out, int64_t B, int64_t per_sample, uint64_t seed, uint32_t stream_id, uint32_t row, uint64_t sample_offset,
               void* stream);
/* tests: the integer half (counters device uint32 [n][4], key host uint32 [2], out device uint32 [n][4]) and the transform
 * (bits device uint32 [n][4] -> out device fp32 [n][4]) on chosen inputs */
int rldm_rng_philox(const uint32_t* counters, const uint32_t key[2], int64_t n, uint32_t* out, void* stream);
int rldm_rng_normals_from_bits(const uint32_t* bits, int64_t n, float* out, void* stream);
/* rldm_sample / rldm_sample_guided with the noise drawn on the device inside the step graph: (seed, draw, sample_offset) stand
 * in place of step_noise, known_noise and renoise_noise, and x_T may be NULL (then drawn with purpose 0, row 0).  Each lane keeps one
 * row buffer [lane batch, out_ch, W, H] per purpose its rows need; a fill launch at the head of every step writes the row that step's
 * scheduler launch reads.  Sample b of the call is sample_offset + b whatever lane runs it.  The three words travel through a
 * 16-byte device record written on the lanes' streams, so a call with another seed or draw replays the same graphs.  The result
 * equals the explicit entry point fed with rldm_randn tensors for the same (seed, draw, purpose, row).  draw < 2^30. */
int rldm_sample_rng(rldm_sampler* s, const float* x_T, uint64_t seed, uint32_t draw, uint64_t sample_offset, const float* cond,
                    float* images, float* latents_out, void* stream);
int rldm_sample_guided_rng(rldm_sampler* s, const float* x_T, uint64_t seed, uint32_t draw, uint64_t sample_offset, const float* known,
                           const float* mask, float* images, float* latents_out, void* stream);
/* tests: how many times the lanes of `s` captured a step graph since creation */
int rldm_debug_sampler_captures(rldm_sampler* s);

/* ---- multi-GPU exchange steps: RCCL over xGMI on the caller's stream (rangeldm_amd/csrc/collective.hip) --
 * One process per GPU.  Rank 0 makes the id and hands its RLDM_UNIQUE_ID_BYTES bytes to the other ranks by any side channel
 * (MPI, a file, torch.distributed's store); every rank then calls rldm_comm_create with its current HIP device set.  RCCL is
 * bound at run time (dlopen): the copy already loaded in the process (PyTorch's) if there is one, else RLDM_RCCL_LIB, else
 * the system librccl. */
#define RLDM_UNIQUE_ID_BYTES 128
typedef struct rldm_comm rldm_comm;
/* binds RCCL and nothing else: what every rank but 0 calls to learn whether it CAN take part (rldm_comm_unique_id would also open
 * ncclGetUniqueId's listening socket and root thread, which only the rank whose id is used should own) */
int rldm_comm_bind(void);
int rldm_comm_unique_id(void* id_out, size_t cap);          /* rank 0 only */
int rldm_comm_create(const void* unique_id, int rank, int world, rldm_comm** out);     /* collective over all ranks */
void rldm_comm_destroy(rldm_comm* c);
int rldm_comm_info(const rldm_comm* c, int* rank, int* world, char* rccl_origin, size_t cap);
/* replaces the per-rank file writing of ldm/inference.py:159-183 as the hand-over of a sample-sharded batch: every rank
 * contributes `count` floats (its finished (B_local, 2, W, H) images, or the x_0 latents) and receives all ranks' buffers in
 * rank order in `all` (world * count floats).  Stream-ordered behind rldm_sample when given the same stream. */
int rldm_allgather_images(rldm_comm* c, const float* local, float* all, int64_t count, void* stream);
/* replaces DDP's gradient exchange (accelerate.prepare(model), ldm/train_unconditional.py:402-404; backward :545): in-place
 * sum (average != 0: mean) over the ranks of `count` floats -- one contiguous bucket of the flat gradient buffer. */
int rldm_allreduce_grads(rldm_comm* c, float* grads, int64_t count, int average, void* stream);

/* ---- range image <-> point cloud (rangeldm_amd/csrc/lidar.hip) ------------------------- */
typedef struct rldm_lidar rldm_lidar;     /* point_cloud_to_range_image replacement, ldm/dataset.py:135-294 */

/* point_cloud_to_range_image.__init__ (ldm/dataset.py:136-154); per-beam tables of the sensor subclasses
 * (ldm/kitti360_range_image.py:19-48, ldm/nuscenes_range_image.py:20-35) are passed to rldm_lidar_create. */
typedef struct rldm_lidar_config {
    int32_t beams;                      /* H = len(incl)                                            */
    int32_t width;                      /* azimuth bins of the projection (`width`, 1024)           */
    int32_t mode;                       /* 0: (r - mean) / std, 1: log2(r + 1) / 6, 2: 1 / r        */
    float mean, std;                    /* 20, 40                                                   */
    float range_fill, intensity_fill;   /* range_fill_value = [100, 0]                              */
    int32_t grid[3];                    /* grid_sizes = [D, H, W] of the BEV volume ([1, 1024, 1024]) */
    float pc_range[6];                  /* [-25.6, -25.6, -3, 25.6, 25.6, 1]                        */
    int32_t normalize_volume_densities; /* log(density + 1)                                         */
} rldm_lidar_config;

int rldm_lidar_create(const rldm_lidar_config* cfg, const float* incl /*host [beams]*/, const float* height /*host*/,
                      rldm_lidar** out);
void rldm_lidar_destroy(rldm_lidar* l);
/* to_pc_torch (ldm/dataset.py:228-278): range_images device fp32 (B, C, W, beams) -> points device fp32
 * [B][W*beams][C > 1 ? 4 : 3] = (x, y, z[, remission]); point index = w * beams + h.  The input is not modified. */
int rldm_lidar_to_points(rldm_lidar* l, const float* range_images, int B, int C, int W, float* points, void* stream);
/* to_voxel (ldm/dataset.py:280-294 over _splat_points_to_volumes :13-132): -> voxel device fp32 (B, 2*D, H, W):
 * D planes of [log(1 +)] vote density, then D planes of density-normalised remission.  C >= 2. */
int rldm_lidar_to_voxel(rldm_lidar* l, const float* range_images, int B, int C, int W, float* voxel, void* stream);
/* to_voxel for training: `voxel` takes the bits rldm_lidar_to_voxel writes, `raw` device fp32 (B, 2*D, H, W) keeps the
 * accumulators before the finalise step: D planes of the vote density d, then D planes of the weighted remission sum S
 * (voxel = log(d + 1) or d | S / max(d, 1e-4)).  The votes are fp32 atomics, as rldm_lidar_to_voxel's. */
int rldm_lidar_to_voxel_train(rldm_lidar* l, const float* range_images, int B, int C, int W, float* raw, float* voxel,
                              void* stream);
/* rldm_lidar_to_voxel_train with an order-fixed splat: per image and cell, with the vote id v = n * 8 + (dx * 4 + dy * 2 + dz)
 * (n = w * beams + h) and the votes that count exactly those the atomic splat casts (pixel touches the volume, corner inside the
 * grid, w != 0), d = ((0.f + w_v1) + w_v2) + ... over the cell's votes in ascending v, S the same over w * f, every + one fp32
 * addition; a cell without votes holds +0.f in both.  `raw` (required) and `voxel` as rldm_lidar_to_voxel_train; the result does
 * not depend on B, on the image's place in the batch, on the launch geometry or on the run.  No floating-point atomics: the
 * votes are sorted by cell with a stable radix sort and summed left to right.  Scratch (kept by the handle, grown on demand):
 * B * (25 * 8 * W * beams + 8 * cells + 1024) bytes.  Refuses 8 * B * W * beams >= 2^31 and grids of 2^31 cells or more.
 * rldm_lidar_to_voxel_backward reads this `raw` as it reads the atomic one. */
int rldm_lidar_to_voxel_ordered(rldm_lidar* l, const float* range_images, int B, int C, int W, float* raw, float* voxel,
                                void* stream);
/* d(loss) / d(range_images) for d(loss) / d(voxel) = dvoxel (B, 2*D, H, W), given the image and the raw accumulators of
 * rldm_lidar_to_voxel_train: dimages device fp32 (B, 2, W, beams), channel 0 the range value's, channel 1 the remission's.
 * Two launches, no atomics: per cell a = gD / (d + 1) [or gD] - [d >= 1e-4] gF S / d^2 and e = gF / max(d, 1e-4) into
 * cell_grad (scratch, the shape of dvoxel); per pixel a gather over its 8 cells, recomputed with the forward's expressions
 * (votes of weight 0 inside the grid included).  0 in both channels where the forward dropped the pixel; 0 in channel 0
 * where the decoded range was negative and replaced by range_fill.  fp32, a fixed operation order: bit-reproducible. */
int rldm_lidar_to_voxel_backward(rldm_lidar* l, const float* range_images, int B, int C, int W, const float* raw,
                                 const float* dvoxel, float* cell_grad, float* dimages, void* stream);
/* `pc[np.linalg.norm(pc[:, :3], 2, axis=1) < max_depth]` per image, order preserved (ldm/inference.py:177-179):
 * points [B][N][cols] -> out [B][N][cols] (first counts[b] rows valid), counts device int32 [B]. cols = 3 or 4. */
int rldm_lidar_filter_points(rldm_lidar* l, const float* points, int B, int N, int cols, float max_depth, float* out,
                             int32_t* counts, void* stream);
/* `(x[b].permute(2, 1, 0).clip(0, 1) * 255).astype(uint8)[:, :, channel]` (ldm/inference.py:180-183):
 * src device fp32 (B, C, W, H) -> dst device bytes [B][H][W] (the pixels of the 8-bit range / BEV PNG). */
int rldm_render_u8(const float* src, int B, int C, int W, int H, int channel, uint8_t* dst, void* stream);
/* point_cloud_to_range_image.__call__ + process_miss_value + normalize + the (2,1,0) permute of
 * RangeDataset.__getitem__ (ldm/dataset.py:159-226, 320-333): one sweep `points` device fp32 [n_points][stride]
 * (x, y, z, intensity, ...) -> image device fp32 (2, width, beams), mask / car_window_mask device bytes
 * (width, beams).  rows: device int32 [n_points] beam index per return, or NULL = nearest inclination
 * (ldm/kitti360_range_image.py:51-61).  min_depth > 0 drops returns with |xyz| <= min_depth
 * (ldm/nuscenes_range_image.py:37-41).  `points` is not modified. */
int rldm_lidar_project(rldm_lidar* l, const float* points, int n_points, int stride, const int32_t* rows, float min_depth,
                       float* image, uint8_t* mask, uint8_t* car_window_mask, void* stream);

/* ---- BEV-histogram evaluation (rangeldm_amd/csrc/metrics.hip) ------------------------------ */
/* load_point_cloud_xyz depth mask (metrics/metrics/histogram/mmd.py:39-44: min_depth < |xyz| < max_depth) +
 * point_cloud_to_histogram(field_size, bins, pc)[0] (histogram.py:4-18, np.histogramdd over +-field_size/2) for a ragged
 * batch: sample s = points[offsets[s] .. offsets[s+1]) (device fp32 [n][stride], device int32 [num_samples + 1])
 * -> hist device uint32 [num_samples][bins][bins] (x bin major).  Counts are exact. */
int rldm_bev_histogram(const float* points, const int32_t* offsets, int num_samples, int stride, float field_size, int bins,
                       float min_depth, float max_depth, uint32_t* hist, void* stream);
/* jsd_2d(sum(hx) / total, sum(hy) / total) (metrics/metrics/histogram/jsd.py:14-16,90-101; scipy jensenshannon, base e).
 * hx / hy device uint32 [n][bins][bins]; *jsd is a HOST double (the call synchronises the stream). */
int rldm_hist_jsd(const uint32_t* hx, int nx, const uint32_t* hy, int ny, int bins, double* jsd, void* stream);
/* np.linalg.norm(x_i / sum(x_i) - y_j / sum(y_j), 2) ** 2 for every pair -- the SPECTRAL norm the `gaussian` kernel of
 * metrics/metrics/histogram/dist_helper.py:84-104 takes of two 2-D pmfs.  lambda device fp32 [nx][ny]; symmetric = 1
 * (hx == hy): only j > i is written, the rest is 0.  bins <= 104, multiple of 4. */
int rldm_hist_spectral_sq(const uint32_t* hx, int nx, const uint32_t* hy, int ny, int bins, int symmetric, float* lambda,
                          void* stream);
/* compute_mmd(samples1, samples2, gaussian, is_hist=True) (dist_helper.py:156-172) with sigma (0.5):
 * out4 HOST doubles = {s1, s2, cross, s1 + s2 - 2 cross} (the call synchronises the stream). */
int rldm_hist_mmd(const uint32_t* hx, int nx, const uint32_t* hy, int ny, int bins, float sigma, double* out4, void* stream);

/* ---- reconstruction metrics (rangeldm_amd/csrc/chamfer.hip) ------------------------------------------------------ */
/* pytorch3d.loss.chamfer_distance (ldm/convert_vae.py:262-271), first half: for a ragged batch of cloud PAIRS
 * (pair p = x[x_offsets[p] .. x_offsets[p+1]) against y[y_offsets[p] .. y_offsets[p+1]); device fp32 [n][stride >= 3], only
 * xyz read; device int32 offsets [num_pairs + 1], starting at 0) the squared distance of every point to its nearest
 * neighbour in the other cloud: x_nn_d2 device fp32 [x_offsets[num_pairs]], y_nn_d2 likewise.  d^2 = ((dx*dx + dy*dy) +
 * dz*dz) in fp32 without contraction: each minimum is bit-equal to that expression evaluated on the CPU.  Every cloud must
 * be non-empty; non-finite coordinates give unspecified results.  The call synchronises the stream. */
int rldm_chamfer_nn(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                    int y_stride, int num_pairs, float* x_nn_d2, float* y_nn_d2, void* stream);
/* second half (point_reduction="mean"): per pair the fp64 mean of each direction, x_mean / y_mean device fp64 [num_pairs];
 * a fixed-order reduction (bit-identical run to run).  CD of pair p = x_mean[p] + y_mean[p]. */
int rldm_chamfer_mean(const float* x_nn_d2, const int32_t* x_offsets, const float* y_nn_d2, const int32_t* y_offsets,
                      int num_pairs, double* x_mean, double* y_mean, void* stream);
/* Nearest neighbour WITH ITS INDEX (rangeldm_amd/csrc/nn_index.hip): pairs packed exactly as rldm_chamfer_nn takes them, same
 * preconditions.  For pair p with clouds X_p (n_p points) and Y_p (m_p points):
 *   x_nn_d2[i]   min over t in Y_p of ((dx*dx + dy*dy) + dz*dz), uncontracted fp32: the bits rldm_chamfer_nn writes
 *   x_nn_idx[i]  the LOWEST index j in [0, m_p) (local to Y_p) whose d2 has exactly those bits
 *   y_nn_d2 / y_nn_idx  the mirror (queries in Y_p, indices local to X_p)
 *   y_hits[j]    how many points of X_p have x_nn_idx == j;  x_hits[i] the mirror.  int32 counts, integer atomics: exact
 * d2 device fp32, idx and hits device int32, each laid out like the packed cloud of its name ([x_offsets[num_pairs]] /
 * [y_offsets[num_pairs]]).  Every value depends on the two clouds of its pair alone: not on the other pairs of the call, not
 * on how a target cloud is split over workgroups (the parts are merged by a 64-bit atomicMin on d2 bits << 32 | index), not
 * on the order of tiles.  Non-finite coordinates give unspecified values, with every index still inside its cloud.
 * The call synchronises the stream. */
int rldm_nn_index(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                  int y_stride, int num_pairs, float* x_nn_d2, int32_t* x_nn_idx, float* y_nn_d2, int32_t* y_nn_idx,
                  int32_t* x_hits, int32_t* y_hits, void* stream);
/* K nearest neighbours (rangeldm_amd/csrc/knn.hip), ONE direction: the queries of pair p against the targets of pair p, both
 * packed as rldm_nn_index takes them (device int32 offsets that start at 0, strides >= 3 with only xyz read, clouds non-empty,
 * coordinates finite).  1 <= K <= RLDM_KNN_MAX_K.  Row i of d2 / idx ([q_offsets[num_pairs]][K], device fp32 / int32) holds the
 * K targets that are smallest in the order (d2 bits, local target index), ascending in that order, with
 * d2 = ((dx*dx + dy*dy) + dz*dz), dx = q - t, uncontracted fp32: equal distances go to the lower index, and for K = 1 the row
 * is rldm_nn_index's answer bit for bit.  exclude_self != 0 requires the two clouds of every pair to have equal sizes and skips
 * the target whose local index is the query's (another point at the same coordinates stays a neighbour at d2 = 0).  A row with
 * fewer than K candidates ends in slots (+inf, -1).  A row depends on the two clouds of its pair alone.  The call
 * synchronises the stream. */
#define RLDM_KNN_MAX_K 32
int rldm_knn(const float* q, const int32_t* q_offsets, int q_stride, const float* t, const int32_t* t_offsets, int t_stride,
             int num_pairs, int K, int exclude_self, float* d2, int32_t* idx, void* stream);
/* PCA surface normals from rldm_knn(exclude_self) indices: idx is [offsets[num_clouds]][K], local to each cloud; entries
 * outside a cloud (-1) are skipped.  Per point, in fp64: the covariance (divided by the count) of the point itself and its
 * valid neighbours about their centroid, a cyclic Jacobi eigen-solve with a fixed number of sweeps, eigenvalues ascending
 * ([N][3]) and as normal ([N][3]) the unit eigenvector of the smallest, oriented towards the sensor at the origin
 * (n . p <= 0; when that is 0 the first non-zero component is positive).  Fewer than two valid neighbours: zeros. */
int rldm_knn_normals(const float* pts, const int32_t* offsets, int stride, int num_clouds, const int32_t* idx, int K,
                     double* normals, double* eigenvalues, void* stream);
/* All-pairs Chamfer matrix between two ragged SETS of clouds, X (nx clouds) and Y (ny clouds), packed as rldm_chamfer_nn
 * takes them (device fp32 [n][stride >= 3], only xyz read; device int32 offsets [nx + 1] / [ny + 1], starting at 0):
 *   xy[i][j] = mean over points q of X_i of min over points t of Y_j of d2(q, t)
 *   yx[i][j] = mean over points t of Y_j of min over points q of X_i of d2(q, t)          CD[i][j] = xy[i][j] + yx[i][j]
 * xy / yx device fp64 [nx][ny].  d2 and every minimum as in rldm_chamfer_nn (bit-equal to the fp32 expression on the CPU);
 * each mean is an fp64 sum of the minima in a fixed order that depends on the two clouds alone (per 2048-point block of
 * the averaged cloud, then the blocks in order), divided once: bit-identical run to run, and identical whether a row is
 * computed in this call or in a call that holds only a block of the rows.  No floating-point atomics.
 * symmetric != 0: Y is X -- the caller passes the SAME buffers, offsets, stride and count; only j > i is computed, the
 * diagonal is 0 and xy[j][i] = yx[i][j], yx[j][i] = xy[i][j] (bit-equal to the rectangular call on (X, X) off the diagonal).
 * Every cloud must be non-empty; non-finite coordinates give unspecified results.  nx * ny < 2^31, and the scratch
 * (2048-point blocks of one set x clouds of the other, fp64) at most 2^28 entries: else an error (rldm_last_error).
 * The call synchronises the stream. */
int rldm_chamfer_matrix(const float* x, const int32_t* x_offsets, int x_stride, int nx, const float* y,
                        const int32_t* y_offsets, int y_stride, int ny, int symmetric, double* xy, double* yx, void* stream);
/* Per row of a device fp64 matrix m [rows][cols] its minimum (min_out device fp64 [rows]) and the LOWEST column index
 * attaining it (arg_out device int32 [rows]): the tie rule the set metrics (COV, 1-NNA) count with.  exclude_diag != 0
 * skips column r of row r; a row left without a column gives +inf / -1.  NaN entries give unspecified results. */
int rldm_matrix_row_argmin(const double* m, int rows, int cols, int exclude_diag, double* min_out, int32_t* arg_out,
                           void* stream);
/* ---- voxel occupancy (rangeldm_amd/csrc/voxel.hip) ------------------------------------------------------------------ */
#define RLDM_VOXEL_RANGE 4               /* return value: a point is out of range (nothing is reported) */
#define RLDM_VOXEL_MAX_SLOTS (1 << 25)   /* workspace bound: hash slots alive at once (256 MiB of keys + 8 MiB of bitmap) */
/* Voxel-occupancy counts of a ragged batch of cloud PAIRS, packed and offset exactly as rldm_chamfer_nn takes them (x the
 * result clouds, y the targets; only xyz read, every cloud non-empty).  With v = voxel as fp32 (positive, finite):
 *   q(c) = floorf(c / v)       one correctly rounded fp32 division, then floor; fp32 denormals are not flushed
 *   a point's voxel is (q(x), q(y), q(z));  it is IN RANGE when -2^20 <= q < 2^20 on every axis (NaN / inf are not)
 *   counts[p] = {a, b, c}:  a = distinct voxels of x_p,  b = distinct voxels of y_p,  c = voxels in both
 * counts device int32 [num_pairs][3].  The integers do not depend on the order of the points, on the other pairs of the call
 * or on how the call is chunked, and equal np.unique(np.floor(c / v), axis=0) on the host.  From them, in fp64:
 *   iou = c / (a + b - c),  precision = c / a,  recall = c / b,  f1 = 2c / (a + b).
 * A call in which ANY point is out of range reports nothing: counts is cleared and the call returns RLDM_VOXEL_RANGE
 * (rldm_last_error says why); a later call works normally.  Pairs are processed in chunks whose hash tables (the power of two
 * >= 2 (n_p + m_p) slots per pair) stay within RLDM_VOXEL_MAX_SLOTS; a single pair that cannot fit (n_p + m_p > 2^24) is an
 * error (return 1, rldm_last_error names it), as is every other failure.  The call synchronises the stream. */
int rldm_voxel_counts(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                      int y_stride, int num_pairs, float voxel, int32_t* counts, void* stream);
/* ---- sensor tables by Hough voting (rangeldm_amd/csrc/hough.hip) --------------------------------------------------- */
#define RLDM_HOUGH_MAX_THETA 65536       /* inclination rows of an accumulator */
#define RLDM_HOUGH_MAX_H 4096            /* height bins of a row (the rows of a workgroup live in 32 KiB of LDS) */
#define RLDM_HOUGH_MAX_BEAMS 256         /* candidate beams of assign / moments */
/* The tables rldm_lidar_create takes (ldm/kitti360_range_image.py:19-48) from the sensor's own sweeps, by the Hough vote of
 * the RangeLDM paper (the reference ships the tables, not the step).  A return of beam k satisfies
 * atan2(height_k - z, d) = incl_k with d = sqrt(x^2 + y^2) (ldm/kitti360_range_image.py:51-61, to_pc_torch,
 * ldm/dataset.py:228-278), so with t = tan(incl): h = z + d t.  Every fp32 expression below is ONE correctly rounded
 * operation, there is no transcendental on the device, and fp32 denormals are kept: numpy restates pack, vote, row_max and
 * assign bit for bit (rangeldm_amd/sensor.py).  n < 2^31 everywhere; n = 0 is a no-op.  All pointers but the tables'
 * arguments are device pointers; nothing synchronises.
 *
 * pack: points device fp32 [n][stride >= 3] -> packed device fp32 [n][2] = (d, z), d = sqrt(x * x + y * y).  A point is
 * valid iff x, y, z are finite and d_min <= d <= d_max; an invalid point is written as d = -1.  Order kept. */
int rldm_hough_pack(const float* points, int64_t n, int stride, float d_min, float d_max, float* packed, void* stream);
/* vote: for every valid packed point and every row i < n_theta:  h = z + d * tan_table[i];  jf = floorf((h - h_min) * inv_dh);
 * acc[i][(int)jf] += 1 iff 0 <= jf < n_h, compared as floats before the cast.  tan_table device fp32 [n_theta] (the host's
 * float32(tan(float64(theta_i)))), acc device uint32 [n_theta][n_h]: added into, never cleared; the caller keeps the number
 * of valid points below 2^32, so no counter wraps.  Integer votes: the result does not depend on any order. */
int rldm_hough_vote(const float* packed, int64_t n, const float* tan_table, int n_theta, float h_min, float inv_dh, int n_h,
                    uint32_t* acc, void* stream);
/* how rldm_hough_vote cuts such a call (host only): rows of one workgroup, points of one slice */
int rldm_hough_vote_shape(int64_t n, int n_theta, int n_h, int32_t* rows, int64_t* slice);
/* per row the largest counter and the lowest bin holding it; a row of zeros gives (0, 0).  Device outputs [n_theta]. */
int rldm_hough_row_max(const uint32_t* acc, int n_theta, int n_h, uint32_t* row_max, int32_t* row_arg, void* stream);
/* assign: candidates device fp32 [beams][2] = (tan_k, h_k), beams <= RLDM_HOUGH_MAX_BEAMS.  Per packed point the residual in
 * tangent space e_k = |(h_k - z) / d - tan_k| (the nearest-inclination rule of ldm/kitti360_range_image.py:51-61 without its
 * atan2); ids[i] = the k of the smallest e_k (ties: the lowest k), or -1 when the point is invalid or that e_k is not < tol.
 * ids device int16 [n]. */
int rldm_hough_assign(const float* packed, int64_t n, const float* candidates, int beams, float tol, int16_t* ids, void* stream);
/* moments: per beam the number of points assigned to it (counts device int64 [beams]) and sums device fp64 [beams][4] =
 * sum d, sum z, sum d^2, sum d z, every value converted to fp64 before any product.  No floating-point atomics; the order of
 * every sum is a function of n alone, so two calls give the same bits. */
int rldm_hough_moments(const float* packed, const int16_t* ids, int64_t n, int beams, int64_t* counts, double* sums,
                       void* stream);
/* ---- Earth Mover's Distance (rangeldm_amd/csrc/emd.hip) ------------------------------------------------------------ */
#define RLDM_EMD_RECT 0          /* every cloud of X against every cloud of Y */
#define RLDM_EMD_SYMMETRIC 1     /* Y is X (the same buffers): j > i computed, mirrored, zero diagonal */
#define RLDM_EMD_DIAGONAL 2      /* nx == ny: only the entries [i][i] (X_i against Y_i) are computed and written */
#define RLDM_EMD_MAX_POINTS 2048
#define RLDM_EMD_BID_CAP 2       /* return value: a pair reached the bid cap (rldm_last_error names it) */
/* All-pairs EMD matrix between two sets of EQUAL-SIZE clouds (1 <= N <= 2048 points each), packed as rldm_chamfer_matrix
 * takes them.  emd[i][j] = (1 / N) sum_i c[i][a(i)] for the assignment a found by an epsilon-scaling forward auction
 * (Gauss-Seidel, one bid at a time, FIFO of unassigned bidders starting as 0 .. N-1, lowest object index on ties):
 *   c[i][j] = sqrtf((dx*dx + dy*dy) + dz*dz) in fp32, no contraction, IEEE sqrt
 *   bid of i:  w[j] = c[i][j] + p[j];  j1 = argmin (lowest j), w2 = min over j != j1 (w2 = w1 for N = 1);
 *              p[j1] = (p[j1] + (w2 - w1)) + e;  i takes j1, j1's previous owner joins the FIFO tail
 *   phases:    e_0 = 0.25f * (largest fp32 side of the joint bounding box of the two clouds), phase k bids with
 *              max(e_k, eps), e_{k+1} = e_k * 0.25f, the phase with e_k <= eps is the last; prices kept, assignments reset
 *   value:     fp64 sum of c[i][a(i)], i ascending, one add after the other, divided once by N
 * so the value, the assignment (assign_out device int32 [nx][ny][N], a permutation), the prices (price_out device fp32
 * [nx][ny][N]) and the number of bids (bids_out device int32 [nx][ny]) depend on the two clouds and eps alone and can be
 * reproduced bit for bit on a CPU; the prices certify emd <= optimum + max_i slack_i (LP duality).  assign_out, price_out
 * and bids_out may be NULL.  emd_out device fp64 [nx][ny].
 * symmetric: RLDM_EMD_RECT, RLDM_EMD_SYMMETRIC (emd_out / bids_out mirrored with a zero diagonal; assign_out / price_out
 * written for j > i only) or RLDM_EMD_DIAGONAL (entries off the diagonal are left untouched).
 * A pair that has made 1024 * N bids with bidders still waiting stops: its value is NaN, the call returns
 * RLDM_EMD_BID_CAP and rldm_last_error names the pair.  Other errors return 1.  The call synchronises the stream. */
int rldm_emd_matrix(const float* x, const int32_t* x_offsets, int x_stride, int nx, const float* y, const int32_t* y_offsets,
                    int y_stride, int ny, int symmetric, float eps, double* emd_out, int32_t* assign_out, float* price_out,
                    int32_t* bids_out, void* stream);
/* ---- farthest point sampling (rangeldm_amd/csrc/fps.hip) ------------------------------------------------------------- */
#define RLDM_FPS_BLOCK 1024              /* lanes of the one workgroup a cloud gets: point i belongs to lane i mod 1024 */
#define RLDM_FPS_RESIDENT_POINTS 65536   /* a cloud's first 64 x 1024 points keep their min-distance in registers */
#define RLDM_FPS_STAGED_POINTS 12288     /* a cloud's first 12 x 1024 points keep their xyz in LDS; the others are re-read */
#define RLDM_FPS_GROUP_POINTS 4096       /* the re-read points are taken in groups of 4 x 1024: four per lane in flight */
#define RLDM_FPS_MAX_POINTS 1048576      /* the largest cloud accepted */
/* Farthest point sampling of every cloud of a ragged batch packed as rldm_chamfer_matrix takes it (x device fp32
 * [n][stride >= 3], only xyz read; offsets device int32 [num_clouds + 1], starting at 0): k indices per cloud, LOCAL to the
 * cloud, in selection order -- idx_out device int32 [num_clouds][k].  start (device int32 [num_clouds], local indices) is
 * the first selected point of each cloud; NULL means 0.  Per cloud, all fp32, one rounding per operation, no contraction:
 *   mind[i] = +inf for every i; sel = start; then k times:
 *     emit sel;  d = ((dx*dx + dy*dy) + dz*dz), dx = x[i] - x[sel] (rldm_chamfer_nn's expression);
 *     mind[i] = min(mind[i], d);  mind[sel] = -inf;  sel = the LOWEST index attaining max_i mind[i]
 * The -inf sentinel keeps a selected index from being selected again: the k indices are distinct, also on clouds full of
 * duplicate points.  The result depends on the cloud, k and start alone (not on the batch or the stride) and equals a
 * sequential CPU evaluation exactly; the indices for k are the first k of those for any larger k.
 * One workgroup per cloud, no atomics.  The min-distances of a cloud's first RLDM_FPS_RESIDENT_POINTS points live in
 * registers; those of the points past them in a workspace of one fp32 per packed point, taken with hipMallocAsync on
 * `stream` for the call and freed before it returns -- only when a cloud is that large.
 * Required, else an error naming the cloud (rldm_last_error): 1 <= k <= points of every cloud <= RLDM_FPS_MAX_POINTS,
 * 0 <= start < points, points * stride * 4 < 2^31, num_clouds * k < 2^31.  Non-finite coordinates give an unspecified
 * selection (still k in-range indices).  The call synchronises the stream. */
int rldm_farthest_point_sample(const float* x, const int32_t* offsets, int stride, int num_clouds, int k, const int32_t* start,
                               int32_t* idx_out, void* stream);
/* ---- Frechet distance over dumped activations (rangeldm_amd/csrc/frechet.hip) --------------------------------------- */
#define RLDM_FRECHET_SWEEP_CAP 2   /* return value: the Jacobi loop ran max_sweeps sweeps and the last still rotated */
#define RLDM_FRECHET_NONFINITE 3   /* return value: an input holds NaN or inf (nothing was computed) */
#define RLDM_FRECHET_MAX_SWEEPS 60 /* the host-side sweep cap rldm_frechet_distance runs with */
/* out [n1][n2] = a . b^T for device fp64 a [n1][d], b [n2][d] on v_mfma_f64_16x16x4_f64; edge tiles are zero filled.
 * K is walked in one ascending order by one workgroup per tile (no split-K, no atomics): an entry depends on its two rows
 * and d alone, whatever tile or call it is computed in. */
int rldm_gram_f64(const double* a, int n1, const double* b, int n2, int d, double* out, void* stream);
/* Singular values of a device fp64 matrix m [rows][cols] by one-sided (Hestenes) Jacobi on the orientation with fewer
 * columns: round-robin pair order (column count padded to even, count - 1 steps per sweep), ONE LAUNCH PER STEP with one
 * workgroup per column pair, no workgroup ever waiting on another.  A pair with |a_p . a_q| <= tol |a_p| |a_q|, or with a
 * zero column, or whose rotation rounds to the identity, is left alone and not counted; tol <= 0 selects
 * sqrt(column length) * 2^-52.  The host reads the count of rotations once per sweep and stops after the first sweep that
 * applied none; *sweeps_out (host, may be NULL) is the number of sweeps
 * run.  After max_sweeps sweeps that all rotated the call returns RLDM_FRECHET_SWEEP_CAP; NaN / inf in m returns
 * RLDM_FRECHET_NONFINITE before the loop.  sv_out device fp64 [min(rows, cols)]: the final column norms, sorted
 * descending.  Every reduction runs in a fixed order: two calls agree bit for bit.  The call synchronises the stream. */
int rldm_singular_values_f64(const double* m, int rows, int cols, double tol, int max_sweeps, double* sv_out,
                             int* sweeps_out, void* stream);
/* Frechet distance between the Gaussians fitted (np.mean, np.cov) to two sets of activations x [n1][d], y [n2][d] (device
 * fp64, n1, n2 >= 2): metrics/metrics/fid/fid_score.py calculate_frechet_distance, without any d x d matrix.  With A, B
 * the centred sets, Tr sqrtm(C1 C2) = |A B^T|_* / sqrt((n1 - 1)(n2 - 1)) (nuclear norm), Tr C1 = sum A^2 / (n1 - 1).
 * out5 (HOST fp64 [5]) = {distance, |mu1 - mu2|^2, Tr C1, Tr C2, Tr sqrtm(C1 C2)}; distance = [1] + [2] + [3] - 2 [4],
 * not clamped at 0.  Return values as rldm_singular_values_f64 (default tol, RLDM_FRECHET_MAX_SWEEPS); the inputs are
 * checked for NaN / inf before anything else.  The call synchronises the stream. */
int rldm_frechet_distance(const double* x, int n1, const double* y, int n2, int d, double* out5, void* stream);
/* Sweeps the Jacobi loop of this thread's last rldm_frechet_distance call ran (0 before the first). */
int rldm_frechet_last_sweeps(void);
/* ---- Kernel distance and precision / recall / density / coverage (rangeldm_amd/csrc/feature_metrics.hip) -------------- */
#define RLDM_FEATURE_MAX_K 16      /* a row keeps its k + 1 smallest squared distances for k up to this */
/* One scan of the rows of a [n_a][d] against the rows of b [n_b][d] (device fp64), folded into per-row outputs without ever
 * forming the n_a x n_b matrix: the reductions that KID's unbiased polynomial-kernel MMD^2 (Binkowski et al. 2018) and
 * precision / recall (Kynkaanniemi et al. 2019) / density / coverage (Naeem et al. 2020; their `prdc` package) are made of.
 * It stands in for `sklearn.metrics.pairwise.polynomial_kernel(degree=3, coef0=1)` row sums and for
 * `scipy.spatial.distance.cdist` followed by `np.argpartition` / `<` / `min` along a row.
 *     g(x, y)   the dot product exactly as rldm_gram_f64 computes it (K ascending in one fixed order, no split-K)
 *     s(x)      g(x, x), taken from that same product path (the diagonal tiles of x . x^T)
 *     d2(x, y)  max(0, (s(x) + s(y)) - 2 g(x, y)), in that order: identical rows are at exactly 0; no square root anywhere
 *     kappa     t = g(x, y) / d + 1; t * t * t                         (degree 3, gamma = 1 / d, coef0 = 1)
 * Outputs (device, each may be NULL and is then not computed; i is a row of a, j a row of b, comparisons strict):
 *     kmin_sq  [n_a][k1] fp64   the k1 smallest d2(a_i, b_j) over j, ascending (k1 = k + 1 <= RLDM_FEATURE_MAX_K + 1, k1 <= n_b;
 *                               NULL exactly when k1 == 0)
 *     count_a  [n_a] int32      #{j : d2 < radius_sq_a[i]}             (given exactly when radius_sq_a [n_a] is)
 *     count_b  [n_a] int32      #{j : d2 < radius_sq_b[j]}             (given exactly when radius_sq_b [n_b] is)
 *     min_sq   [n_a] fp64       min_j d2
 *     poly_sum [n_a] fp64       sum_j kappa(a_i, b_j) (given exactly when poly != 0); with exclude_diagonal without
 *                               j == i + row_offset
 * The columns are cut into chunks of rldm_feature_scan_column_chunk(n_b) = 64 * ceil(ceil(n_b / 64) / 16) rows of b (at most
 * 16 chunks, a function of n_b alone).  poly_sum is the sum over ascending chunks of each chunk's sum over ascending j; the
 * other outputs do not depend on the order.  A row's outputs depend on that row, on b and on row_offset alone: a slice of a
 * scanned on its own gives those rows of the whole scan bit for bit.  Workspace: n_a + n_b fp64 for the norms and, with more
 * than one chunk, the outputs once per chunk -- O(n_a + n_b).  NaN / inf in a, b or a radius returns RLDM_FRECHET_NONFINITE
 * before anything else runs (that check synchronises the stream; the scan itself is only enqueued). */
int rldm_feature_scan_f64(const double* a, int n_a, const double* b, int n_b, int d, int k1, const double* radius_sq_a,
                          const double* radius_sq_b, int poly, int exclude_diagonal, long long row_offset, double* kmin_sq,
                          int32_t* count_a, int32_t* count_b, double* min_sq, double* poly_sum, void* stream);
/* The column chunk rldm_feature_scan_f64 uses for n_b rows of b (0 for n_b <= 0). */
int rldm_feature_scan_column_chunk(int n_b);
/* ---- RangeNet++ inference (rangeldm_amd/csrc/rangenet.hip) ---------------------------------------------
 * The DarkNet21 / DarkNet53 segmentation network the FRD activations and the IoU / accuracy metrics come from.  Activations
 * are device bf16 channels-last [B][H][W][pitch(C)], pitch(C) = RLDM_RN_PITCH(C) (pad channels hold zeros).  One layer is
 *     acc = sum_taps W . X              zeros outside the image on both axes (no wrap)
 *     v   = acc * scale[c] + shift[c]   fp32; BatchNorm (eval) and bias folded by the caller
 *     v   = v >= 0 ? v : 0.1f * v       if leaky
 *     v   = v + add0 + add1             optional bf16 tensors of the output's shape, in that order, fp32
 *     out = bf16(v)                     round to nearest even
 * on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; every step after the sum is one fp32 operation (no FMA). */
enum rldm_rangenet_kind {
    RLDM_RN_CONV1X1 = 0,        /* 1x1                                                                                   */
    RLDM_RN_CONV3X3 = 1,        /* 3x3, stride (1,1), padding 1                                                          */
    RLDM_RN_CONV3X3_S2 = 2,     /* 3x3, stride (1,2) along W, padding 1: W_out = (W - 1) / 2 + 1                         */
    RLDM_RN_UPCONV = 3          /* ConvTranspose2d kernel [1,4], stride [1,2], padding [0,1]: W_out = 2 W, run as two
                                 * 2-tap convs by output-column parity                                                   */
};
#define RLDM_RN_PITCH(c) (((c) + 15) & ~15)
typedef struct rldm_rangenet_layer_desc {
    int32_t kind;               /* enum rldm_rangenet_kind */
    int32_t B, H, W;            /* the INPUT's batch, rows and columns */
    int32_t Cin, Cout;
    int32_t leaky;              /* LeakyReLU(0.1) after the affine */
} rldm_rangenet_layer_desc;
typedef struct rldm_rangenet_config {
    int32_t layers;             /* 21 or 53 (the block counts per encoder stage) */
    int32_t in_channels;        /* 5: range, x, y, z, remission */
    int32_t num_classes;        /* 20 */
} rldm_rangenet_config;
typedef struct rldm_rangenet rldm_rangenet;
/* bf16 elements of a layer's packed weight image (-1: bad arguments), and the packing itself, on the host:
 * w fp32 [Cout][T][Cin] with T = 1 (1x1), 9 (3x3, tap = 3 ky + kx) or 4 (up-conv, tap = kx) -> packed [panel of 32 output
 * channels][16 input channels][T][lane 64][8], the MFMA's A fragment per lane, zero padded; rounded to bf16 (nearest even). */
long long rldm_rangenet_packed_elems(int kind, int Cin, int Cout);
int rldm_rangenet_pack_weights(int kind, int Cin, int Cout, const float* w, uint16_t* packed);
/* One layer, one launch (the network walk calls exactly this).  x device bf16 [B][H][W][pitch(Cin)]; w_packed device;
 * scale / shift device fp32 [Cout]; add0 / add1 device bf16 of the output's shape or NULL.  Outputs, each optional (at least
 * one): out device bf16 [B][H][W_out][pitch(Cout)]; out_f32 device fp32 (B, Cout, H, W_out), v before the rounding;
 * gathered device fp32 (B, n_gather): v at the positions of one image's (Cout, H, W_out) flattening whose bit is set in
 * gather_mask (uint32 words, bit i & 31 of word i >> 5), written to column gather_slot[i]; argmax device uint8 (B, H, W_out):
 * the channel of the largest v, lowest index on ties (Cout <= 32).  Every tensor must stay below 2^31 elements. */
int rldm_rangenet_layer(const rldm_rangenet_layer_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                        const void* add0, const void* add1, void* out, float* out_f32, const uint32_t* gather_mask,
                        const int32_t* gather_slot, int n_gather, float* gathered, uint8_t* argmax, void* stream);
/* The layers of an architecture in walk order: stem; enc1..enc5 (down-sampler, then conv1 / conv2 of every BasicBlock);
 * dec5..dec1 (up-conv, conv1, conv2); head.  layer_info fills kind / Cin / Cout / leaky (B, H, W are zero). */
int rldm_rangenet_num_layers(const rldm_rangenet_config* cfg);
int rldm_rangenet_layer_info(const rldm_rangenet_config* cfg, int index, rldm_rangenet_layer_desc* out);
/* weights / scale / shift: n_layers HOST pointers in walk order (fp32 [Cout][T][Cin], [Cout], [Cout]); packed and uploaded here. */
int rldm_rangenet_create(const rldm_rangenet_config* cfg, const float* const* weights, const float* const* scale,
                         const float* const* shift, int n_layers, rldm_rangenet** out);
void rldm_rangenet_destroy(rldm_rangenet* net);
/* proj device fp32 (B, in_channels, H, W), W a multiple of 32.  skips[os] is the input of each down-sampler; each decoder
 * stage is up-conv -> BasicBlock -> + skips[os]; dropout is the identity.  features: n_gather == 0: device fp32 (B, 32, H, W)
 * or NULL; n_gather > 0: device fp32 (B, n_gather), see rldm_rangenet_layer.  argmax device uint8 (B, H, W) and / or logits
 * device fp32 (B, num_classes, H, W).  The net owns its activation arena (grown on demand; one forward per net at a time). */
int rldm_rangenet_forward(rldm_rangenet* net, const float* proj, int B, int H, int W, const uint32_t* gather_mask,
                          const int32_t* gather_slot, int n_gather, float* features, uint8_t* argmax, float* logits, void* stream);
/* ---- RangeNet++ around the forward (rangeldm_amd/csrc/rangenet_post.hip) ----------------------------------
 * A ragged batch of B scans, packed as rldm_farthest_point_sample takes it: points device fp32 [sum N][stride >= 3] (x, y, z,
 * and remission when stride >= 4, else 0), offsets device int32 [B + 1] starting at 0.  Neither call reads the offsets on the
 * host, allocates or synchronises: everything is queued on `stream`.
 *
 * rldm_rangenet_project: LaserScan.do_range_projection and the parser's normalisation (modules/kittiparser.py:111-171,
 * 391-395), each step one fp32 operation in the reference's order (atan2f / asinf are the device's):
 *   depth = sqrt((x*x + y*y) + z*z);  yaw = -atan2(y, x);  pitch = asin(z / depth)
 *   px = clamp(floor(0.5 * (yaw / pi + 1) * W), 0, W - 1);  py = clamp(floor((1 - (pitch + |fov_down|) / fov) * H), 0, H - 1)
 * fov_up / fov_down in degrees; the radians are computed in fp64 and rounded once, as numpy does with python floats.
 * A pixel goes to its NEAREST point, among equal depths to the LOWEST index (atomicMin on depth bits << 32 | index into
 * keys_workspace, device uint64 (B, H, W), which the call initialises itself).  A point whose depth is 0 or not finite does
 * not compete and gets px = py = -1.  Outputs, all device, all but proj optional (NULL):
 *   proj fp32 (B, 5, H, W)      ((value - means[c]) / stds[c]) * mask for range, x, y, z, remission; an empty pixel's value is -1
 *   mask fp32 (B, H, W)         proj_idx > 0: the pixel point 0 wins is dropped too (the reference's quirk)
 *   proj_range fp32 (B, H, W)   the winner's depth, -1 where empty;  proj_idx int32 (B, H, W): its index in its cloud, or -1
 *   px, py int32 [sum N], unproj_range fp32 [sum N]: per point
 * means / stds: HOST fp32 [5] (read before the call returns). */
int rldm_rangenet_project(const float* points, const int32_t* offsets, int B, int stride, int H, int W, double fov_up,
                          double fov_down, const float* means, const float* stds, uint64_t* keys_workspace, float* proj,
                          float* mask, float* proj_range, int32_t* proj_idx, int32_t* px, int32_t* py, float* unproj_range,
                          void* stream);
/* Per-point labels from the per-pixel argmax (device uint8 (B, H, W)): labels device uint8 [sum N].  A point with px < 0 gets 0.
 * knn == 0: labels = argmax[py, px] (proj_range, unproj_range, weights may be NULL).
 * knn > 0: postproc/KNN.py forward.  The window is search x search around (py, px), entry k = dy * search + dx, no azimuth
 * wrap; an entry outside the image has range 0 and label 0 (F.unfold's zero padding); an in-image range < 0 becomes +inf; the
 * centre's range is the point's own unproj_range; distance = |entry - unproj_range| * weights[k] (weights device fp32
 * [search * search], the caller's 1 - gaussian).  The knn smallest distances vote, ties to the lowest k; with cutoff > 0 an
 * entry farther than cutoff votes for nobody; the label is the class in [1, num_classes) with the most votes, the lowest on
 * ties, 1 without votes.  Required, else an error: search odd and at most 7, knn <= search * search, 2 <= num_classes <= 32,
 * cutoff >= 0. */
int rldm_rangenet_unproject(const float* proj_range, const uint8_t* argmax, const int32_t* px, const int32_t* py,
                            const float* unproj_range, const int32_t* offsets, int B, int H, int W, int knn, int search,
                            const float* weights, float cutoff, int num_classes, uint8_t* labels, void* stream);

/* Range-image errors (ldm/convert_vae.py:236-247 MAE / PSNR; metrics/metrics/mae.py:45-117 range MAE): a, b device fp32
 * (B, C, W, H), C <= 8.  Per image, over the channels of channel_mask and the azimuth columns (w0 + k) mod W,
 * k in [0, w1 - w0) (0 <= w0 < W, w0 < w1 <= w0 + W: the window may wrap past the seam), with v -> v * scale[c] + shift[c]
 * (scale / shift HOST fp32 [C]) applied to both images in fp64: abs_sum / sq_sum device fp64 [B] = sum |a' - b'| and
 * sum (a' - b')^2, fixed-order reductions.  The caller divides by the pixel count. */
int rldm_range_errors(const float* a, const float* b, int B, int C, int W, int H, int channel_mask, const float* scale,
                      const float* shift, int w0, int w1, double* abs_sum, double* sq_sum, void* stream);
#define RLDM_UPSAMPLE_NEAREST 0   /* cv2 INTER_NEAREST: source row floor(r / rate) */
#define RLDM_UPSAMPLE_BICUBIC 1   /* cv2 INTER_CUBIC restated: src = (r + 0.5) / rate - 0.5, Keys A = -0.75, rows clamped */
/* The beam-upsampling baselines of metrics/metrics/mae.py:61-81 (cv2.resize(target[::rate], fx=1, fy=rate)): src device
 * fp32 (B, C, W, Hs) -> dst device fp32 (B, C, W, Hs * rate) along the beam (last) axis. */
int rldm_beam_upsample(const float* src, int B, int C, int W, int Hs, int rate, int mode, float* dst, void* stream);

/* ---- UNet training step (rangeldm_amd/csrc/train*.hip, mapped in DESIGN.md 3; ldm/train_unconditional.py:466-558) ----
 * Op-level entry points driven by rangeldm_amd/training.py (the autograd tape is host-side).  Every tensor is device
 * fp32, activations / gradients channels-last [B][W][H][C] (W wraps, H zero-pads); GEMM operands are rounded to bf16 into
 * the MFMA with fp32 accumulation (the reference's `mixed_precision: bf16`). */
typedef struct rldm_train_conv_desc {
    int32_t B, Win, Hin, Cin;   /* input tensor                                                                    */
    int32_t N;                  /* output channels                                                                 */
    int32_t taps;               /* 9: 3x3 pad 1 (ldm/utils.py:40-55), 1: 1x1 / Linear                             */
    int32_t stride;             /* 1 | 2 (Downsample2D, ldm/utils.py:107-116)                                      */
    int32_t mode;               /* 0 plain, 1 nearest-x2 of the input first (Upsample2D), 2 zero insertion (data
                                   gradient of a stride-2 conv); output = (Win << (mode != 0)) / stride;
                                   | RLDM_TRAIN_PAD_END: end-only padding (below)                                  */
} rldm_train_conv_desc;
/* End-only padding, the VAE encoder's down-sampler (vae/sgm/.../model.py:164-172: one wrapped column behind W, one zero row
 * behind H, then 3x3 stride 2 without padding), as a flag in `mode` -- the struct keeps its size.  Valid for 9 taps with
 * stride 2, mode 0 (forward and weight gradient: output (wo, ho) under tap (dw, dh) in {-1, 0, 1}^2 reads the virtual pixel
 * (2 wo + dw + 1, 2 ho + dh + 1); W wraps, row Hin is zero) and with stride 1, mode 2 (the data gradient: the zero-insertion
 * conv over dy with the transposed, flipped weight copy reads (v + d - 1); W wraps in the zero-inserted space, a negative row
 * is zero).  Anything else with the flag is a "bad conv desc"; without it every launch is what it was.  The fused and all-taps
 * kernels have no such instance (_fused_ok: 0); rldm_train_conv_splits treats the desc like its symmetric twin. */
#define RLDM_TRAIN_PAD_END 4
/* y = conv(x) + bias + rowadd[b] + res (each optional); w_packed = bf16 [N][taps][ceil16(Cin)] from
 * rldm_train_pack_weights (forward copy, or the transposed copy with Cin/N swapped for the data gradient). */
int rldm_train_conv(const rldm_train_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* rowadd,
                    int rowadd_ld, const float* res, float* y, int accumulate, void* stream);
/* How many K splits rldm_train_conv uses for this shape (1: none).  A split launch adds its partial tiles to y atomically
 * after zero-filling it; with accumulate != 0 it adds onto what y holds, so a caller that owns pre-zeroed outputs (one fill
 * for all of a step's split launches) passes accumulate = 1 and saves the per-launch fill. */
int rldm_train_conv_splits(const rldm_train_conv_desc* d, int rowadd_ld);
/* dw[N][Cin][taps] += sum over pixels of dy (x) x  (torch weight layout; dw must be zeroed by the caller). */
int rldm_train_wgrad(const rldm_train_conv_desc* d, const float* dy, const float* x, float* dw, void* stream);
/* The same plus the bias / per-image row gradients of rldm_train_colsum from the same pass over dy (rows / total may be NULL);
 * inside the all-taps kernel the sums are taken from the staged bf16 tile. */
int rldm_train_wgrad_bias(const rldm_train_conv_desc* d, const float* dy, const float* x, float* dw, float* rows, int rows_ld,
                          int rows_accumulate, float* total, void* stream);
/* rows[b][n] (+)= sum over image b's pixels of dy[p][n] (time-embedding row gradient); total[n] += over all images (bias). */
int rldm_train_colsum(const float* dy, int B, int npix, int N, float* rows, int rows_ld, int rows_accumulate, float* total,
                      void* stream);
/* GroupNorm (+ SiLU): stats [B][groups][2] = (mean, rstd) are written by forward and read by backward. */
int rldm_train_gn_forward(const float* x, int B, int npix, int C, int groups, float eps, const float* gamma, const float* beta,
                          int silu, float* stats, float* y, void* stream);
int rldm_train_gn_backward(const float* x, const float* dy, const float* stats, int B, int npix, int C, int groups,
                           const float* gamma, const float* beta, int silu, float* scratch /*[B][groups][2]*/, float* dx,
                           int accumulate, float* dgamma, float* dbeta, void* stream);
/* ---- fused tape (round 5): GroupNorm never runs as a tensor pass of its own ----------------------------------------------
 * A tensor's GroupNorm statistics travel as per-(image, channel) pairs cs [B][C][2] = (sum, sum of squares), accumulated
 * (atomically, into a buffer the caller zeroed) by the epilogue of the conv that produced the tensor.  Consumers rebuild
 * act(GroupNorm(x)) from x + cs while they stage x -- the reference's `F.silu(norm(x))` in front of every ResnetBlock2D conv
 * and `group_norm(x)` in front of to_q/k/v (sgm model.py:93-125, diffusers ResnetBlock2D / Attention) -- and a concatenated
 * input (`torch.cat([h, skip], 1)` of the up blocks) is read from its two sources in place.  Backward: the data-gradient conv
 * whose output is d act(GN(g)) turns it into dz = dy act'(z) in its epilogue and accumulates gs [B][C][2] = (sum dz, sum dz
 * xhat); rldm_train_gn_backward_apply finishes dx (+ residual gradient, split over the two sources) and d gamma / d beta. */
typedef struct rldm_train_fuse {
    /* input side (conv, wgrad: the `x` operand) */
    const float* x1;            /* second source: channels [C0, Cin) of the input (NULL: `x` holds all Cin)                */
    int32_t C0;                 /* channels of `x` when x1 != NULL (a multiple of 64 -- 32 when Cin % 64 != 0)             */
    const float* cs0;           /* (sum, sumsq) pairs of x / x1; cs0 == NULL: the input is used as it is                   */
    const float* cs1;
    const float* gamma;         /* GroupNorm affine over the Cin channels                                                  */
    const float* beta;
    int32_t silu, groups;
    float eps;
    /* output side (conv only; at most one of the two) */
    float* cs_out;              /* += (sum, sumsq) of y per (image, channel): [B][N][2]                                    */
    const float* g0;            /* data gradient: y = d act(GN(cat(g0, g1))); stored as dz, gs_out [B][N][2] += sums       */
    const float* g1;
    int32_t G0;                 /* channels of g0 when g1 != NULL                                                          */
    const float* gcs0;          /* (sum, sumsq) pairs of g0 / g1                                                           */
    const float* gcs1;
    const float* ggamma;
    const float* gbeta;
    int32_t gsilu, ggroups;
    float geps;
    float* gs_out;
} rldm_train_fuse;
/* rldm_train_conv with the above folded in.  prezeroed: as `accumulate` of rldm_train_conv for split launches (y is a zeroed
 * buffer of the caller); a fused epilogue never adds onto an existing y.  _ok: 1 if the shape has a fused instance. */
int rldm_train_conv_fused_ok(const rldm_train_conv_desc* d, const rldm_train_fuse* f, int rowadd_ld);
int rldm_train_conv_fused(const rldm_train_conv_desc* d, const rldm_train_fuse* f, const float* x, const void* w_packed,
                          const float* bias, const float* rowadd, int rowadd_ld, const float* res, float* y, int prezeroed,
                          void* stream);
/* rldm_train_wgrad_bias with x = act(GN(cat(x, x1))) rebuilt while staging (input side of `f` only). */
int rldm_train_wgrad_fused_ok(const rldm_train_conv_desc* d, const rldm_train_fuse* f);
int rldm_train_wgrad_fused(const rldm_train_conv_desc* d, const rldm_train_fuse* f, const float* dy, const float* x, float* dw,
                           float* rows, int rows_ld, int rows_accumulate, float* total, void* stream);
/* The all-taps weight-gradient kernel leaves partial tiles that a reduction adds into dw.  With deferral on, that reduction is not
 * launched on its own: it rides (as extra workgroups) on the next rldm_train_conv / _conv_fused launch on the same stream -- the
 * data gradient of the same layer, which does not depend on it -- or is launched by whatever comes first of: the next weight-gradient
 * call, rldm_train_flush_reduce, rldm_train_defer_reduce(0).  Call rldm_train_flush_reduce before anything else reads dw. */
int rldm_train_defer_reduce(int on);
int rldm_train_flush_reduce(void);
int rldm_train_reduce_pending(void);   /* 1 while a deferred reduction waits for a launch to ride on (tests) */
/* (round 6) Grouped weight gradients.  The weight gradients of a step (`loss.backward()`, ldm/train_unconditional.py:545) depend on
 * nothing behind them in the backward pass and nothing in it depends on them.  With grouping on, rldm_train_wgrad_bias / _wgrad_fused
 * calls that the all-taps kernel covers are QUEUED (their dy / x / statistics operands must stay alive and unmodified), and
 * rldm_train_wgrad_group_flush -- or group(0), or a queued call on another stream -- runs the queue as a handful of launches that each
 * compute up to 22 layers (block id -> layer, tile, K slice; the K slices of a tile are summed in slice order by the tile's last
 * arriver: no reduction launches, bit-reproducible gradients).  A dw may be queued again: the call flushes the queue first, so its
 * gradients add in call order.  dw / rows / total are final only after the flush, which empties the queue even when it fails.  One
 * caller thread. */
int rldm_train_wgrad_group(int on);
int rldm_train_wgrad_group_flush(void);
int rldm_train_wgrad_group_pending(void);   /* queued layers (tests) */
/* Deterministic mode: a process-wide switch for one caller thread, read when a call is enqueued (so a captured graph keeps the mode
 * it was captured in).  _enabled returns the current value.  With the switch on, the outputs of every rldm_train_* entry point are a
 * function of its inputs and shapes alone, bit for bit: no floating-point atomics (global or LDS) run, every sum that crosses
 * workgroups goes through partial rows in scratch that are added in index order, nothing depends on workgroup arrival order, on other
 * streams or on graph replay.  It costs launches and speed; default-mode arithmetic is untouched.  What changes:
 *   conv / conv_fused      never split K (rldm_train_conv_splits returns 1): one workgroup contracts all of K in stage order.
 *   GroupNorm statistics   ONE canonical order for the (sum, sumsq) pair of an (image, channel), whoever produces it -- the epilogue
 *                          of rldm_train_conv_fused for its stored y, or rldm_train_chan_stats:  pixel index p = w * H + h inside the
 *                          image; partial t covers pixels [64 t, 64 t + 64) (the last one may be short); inside a partial, lane k of
 *                          16 starts from +0 and adds x[p] (sumsq: the fp32-rounded product x[p] * x[p], never fused with the sum) for
 *                          p = 64 t + k + 16 j, j = 0, 1, 2, 3; the partial is ((((0 + lane 0) + lane 1) + ...) + lane 15); the pair is
 *                          (((0 + partial 0) + partial 1) + ...) and is ADDED to what cs holds.  The (sum dz, sum dz xhat) pairs of a
 *                          data-gradient epilogue (gs_out) follow the same order.  train_ops.chan_stats_host restates it in numpy.
 *   colsum, and the rows / total of wgrad_bias / wgrad_fused (which then sum the fp32 dy, not the staged bf16 tile)
 *                          slab z covers pixels [256 z, 256 z + 256) of an image; lane k of 16 adds pixels 256 z + k + 16 j in order
 *                          of j; lanes added k = 0 .. 15; image sum = slabs added in order; rows[b] (+)= image sum; total += the image
 *                          sums added b = 0 .. B - 1 (from +0).
 *   weight gradients       always partial tiles per K slice, added in slice order (no atomics into dw).
 *   gn_forward / backward  the one-block-per-(image, group) kernels at every size; d gamma / d beta per image, added in image order.
 *   mse / sqnorm           block i's fp64 partial as in the default mode (mse: element i * 256 + t per thread; sqnorm: thread t of
 *                          block i adds g[(i + j nb) * 256 + t]^2 in order of j, nb = min(ceil(n / 256), 2048) blocks), a block's 256
 *                          values added as a binary tree (lanes l and l ^ 32, then ^ 16 .. ^ 1, then the four waves in order); the
 *                          result = the same two steps over the block partials (thread t adds partials t, t + 256, ... first).
 *   l1                     mse's partials and folds, for the loss and for each channel's absolute-error sum (see rldm_train_l1).
 *   gaussian               mse's partials and folds for the KL sum (see rldm_train_gaussian); z and the backward are element-wise.
 *   disc_conv / _dgrad     no split across workgroups: the four waves of a tile's workgroup take a quarter of the taps each, in tap
 *                          order, and are added ((w0 + w1) + w2) + w3 (both modes).
 *   disc_wgrad             partial tiles per K slice, added in slice order (both modes); dbias is colsum's.
 *   disc_bn_forward / _backward   fp64 partials per 256 rows, added in index order (both modes); no atomics.
 *   disc_hinge / _generator       l1's partials and folds (see rldm_train_disc_hinge); the gradients are element-wise.
 *   disc_lrelu / _adaptive_mix    element-wise.
 *   meta_forward / _backward      GEMM reductions cut into K slices leave partial tiles that are added in slice order, the gathers
 *                          (dx, dr) add their rows in a fixed order (both modes); the three bias sums are colsum's.
 *   meta_range / _range_grad      element-wise.
 * The RCCL all-reduce of a multi-rank step is outside this guarantee. */
int rldm_train_deterministic(int on);
int rldm_train_deterministic_enabled(void);
/* cs [B][C][2] += (sum, sumsq) per (image, channel) of x [B][npix][C]: for tensors no fused conv produced. */
int rldm_train_chan_stats(const float* x, int B, int npix, int C, float* cs, void* stream);
/* dx = rstd (gamma dz - mean_g(gamma dz) - xhat mean_g(gamma dz xhat)) + res, the GroupNorm over cat(x0, x1) [C0 | C - C0
 * channels]; written (accumulate == 0) or added to dx0 / dx1; dgamma[c] += sum_b gs[b][c].y, dbeta[c] += sum_b gs[b][c].x
 * (both may be NULL).  res: [B][npix][C] or NULL. */
int rldm_train_gn_backward_apply(const float* dz, const float* x0, const float* x1, int C0, const float* cs0, const float* cs1,
                                 const float* gs, int B, int npix, int C, int groups, float eps, const float* gamma,
                                 const float* res, float* dx0, int accumulate0, float* dx1, int accumulate1, float* dgamma,
                                 float* dbeta, void* stream);
/* Linear layers on B <= 16 rows (TimestepEmbedding MLP, ResnetBlock2D.time_emb_proj): y[b][n] (+)= sum_k x[b][k]
 * W[n][k] + bias[n] with W the packed bf16 copy [N][ceil16(K)] (forward copy; the transposed copy gives the data gradient);
 * x / y rows may be slices of wider matrices (ldx / ldy in floats).  _wgrad: dw [N][K] fp32 += dy^T x, dbias[n] += sum_b dy. */
int rldm_train_linear_rows(const float* x, int ldx, const void* w_packed, int K, const float* bias, float* y, int ldy, int B, int N,
                           int accumulate, void* stream);
int rldm_train_linear_rows_wgrad(const float* dy, int ldy, const float* x, int ldx, int B, int N, int K, float* dw, float* dbias,
                                 void* stream);
/* softmax(q k^T / sqrt(8)) v per head of 8 channels; q, k, v, o [B][L][C]; lse / delta [B][C/8][L]. */
int rldm_train_attention_forward(const float* q, const float* k, const float* v, int B, int L, int C, float* o, float* lse,
                                 void* stream);
int rldm_train_attention_backward(const float* q, const float* k, const float* v, const float* o, const float* dO, const float* lse,
                                  int B, int L, int C, float* delta, float* dq, float* dk, float* dv, void* stream);
/* The same with q, k, v the three thirds of ONE projection output qkv [B][L][3C] (to_q / to_k / to_v fused into one 1x1 conv
 * with 3C outputs) and dq, dk, dv the thirds of dqkv [B][L][3C]; o, dO [B][L][C]. */
int rldm_train_attention_qkv_forward(const float* qkv, int B, int L, int C, float* o, float* lse, void* stream);
int rldm_train_attention_qkv_backward(const float* qkv, const float* o, const float* dO, const float* lse, int B, int L, int C,
                                      float* delta, float* dqkv, void* stream);
int rldm_train_add(const float* a, const float* b, float* y, int64_t n, void* stream);
int rldm_train_copy_channels(const float* src, int src_ld, int src_off, float* dst, int dst_ld, int dst_off, int ncopy,
                             int64_t npix, int accumulate, void* stream);
int rldm_train_sum2x2(const float* du, int B, int W, int H, int C, float* dx, void* stream);       /* nearest-x2 backward */
int rldm_train_silu(const float* x, const float* dy, float* y, int64_t n, int backward, int accumulate, void* stream);
int rldm_train_timestep_embedding(const int64_t* timesteps /*device*/, int B, int dim, float* out, void* stream);
/* (B, C, W, H) fp32 + optional pos-encoding channel (ldm/train_unconditional.py:455-463,500-501) -> [B][W][H][C(+1)] */
int rldm_train_pack_input(const float* x, int B, int C, int W, int H, int pos_encoding, float* y, void* stream);
int rldm_train_unpack_output(const float* x, int B, int C, int W, int H, float* y, void* stream);
/* F.mse_loss(model_output, target) with optional per-sample weights (min-SNR, :529-543): pred [B][W][H][C], target
 * (B, C, W, H); dpred [B][W][H][C]; *loss device double. */
int rldm_train_mse(const float* pred, const float* target, const float* weight, int B, int C, int W, int H, float* dpred,
                   double* loss, void* stream);
/* The VAE's reconstruction term before the discriminator starts (channel-weighted L1, summed, divided by the batch):
 *   loss = (1 / B) sum_{b,w,h,c} wc[c] |pred[b][w][h][c] - target[b][c][w][h]|
 * pred [B][W][H][C], target (B, C, W, H), wc device [C] (C <= 16); dpred [B][W][H][C] = s g[c] with s = -1 / 0 / +1 the sign of
 * the fp32 difference (0 at equality) and g[c] = wc[c] / B one fp32 division: every element is one exact product.  out: device
 * double [1 + C] = (loss, the unweighted sum of |difference| per channel).  fp64 sums like rldm_train_mse: element i * 256 + t
 * (NHWC order) is lane t of partial i, a partial's 256 values are added as mse's binary tree, the partials meet in fp64 atomics
 * -- or, in the deterministic mode, are folded as mse's are (channel k's partial takes +0 from the other channels' lanes).
 * train_ops.l1_host restates it in numpy. */
int rldm_train_l1(const float* pred, const float* target, const float* wc, int B, int C, int W, int H, float* dpred, double* out,
                  void* stream);
/* The VAE's posterior (vae/sgm/modules/distributions/distributions.py:24-64, DiagonalGaussianRegularizer): moments
 * [B][W][H][2 Z] NHWC, mean in channels [0, Z), logvar in [Z, 2 Z); noise (B, Z, W, H) or NULL (sample_posterior = False: z = mean).
 *   lc = clamp(logvar, -30, 20);  z[b][w][h][c] = mean + expf(0.5 lc) noise  (fp32);
 *   *kl (device double) = (1 / B) sum 0.5 (mean^2 + exp(lc) - 1 - lc), fp64 per element, summed like rldm_train_l1's loss: element
 *   i * 256 + t of z is lane t of partial i, the partials meet in an fp64 atomic -- or, in the deterministic mode, are folded as
 *   mse's are.
 * _backward, for loss = rec + kl_weight kl and kw = kl_weight / B: dmoments [B][W][H][2 Z],
 *   dmean = dz + kw mean;  dlogvar = pass (dz noise 0.5 expf(0.5 lc) + kw 0.5 (expf(lc) - 1)),  pass = (-30 <= logvar <= 20), both
 *   ends included (torch.clamp's gradient); noise NULL drops the first term.  train_ops.gaussian_host restates both in numpy. */
int rldm_train_gaussian(const float* moments, const float* noise, int B, int W, int H, int Z, float* z, double* kl, void* stream);
int rldm_train_gaussian_backward(const float* moments, const float* noise, const float* dz, float kw, int B, int W, int H, int Z,
                                 float* dmoments, void* stream);
/* Decoder-guided sampling (csrc/guide.hip; rangeldm_amd/guidance.py restates each entry point in numpy): the measurement-consistency
 * step on the clean-latent estimate z0 of a DDIM step.  Plain fp32, one rounding per stated operation (no contraction), for every
 * setting of rldm_train_deterministic.
 * _residual: xhat [B][W][H][C] (the tape decoder's reconstruction), y (B, C, W, H) the known image, m (B, 1, W, H) fp32 (> 0.5: known),
 *   wc device [C].  d = xhat - y;  gx [B][W][H][C] = (2 wc[c]) d where known (one product: 2 wc[c] is exact), +0 elsewhere;
 *   L device double [B], L[b] = sum over image b of wc[c] d d where known, fp64 per element, in ONE order at every call: element
 *   256 i + t of the image (NHWC order) is lane t of partial i, a partial's 256 values are added as rldm_train_mse's binary tree, and the
 *   image's partials are folded as mse's are (thread t adds partials t, t + 256, ... first).  No floating-point atomics.
 * _latent:   zin [B][W][H][C] = z0 (B, C, W, H) * inv_sf: the decoder's input (inv_sf = 1 / scaling_factor rounded to fp32 by the caller).
 * _update:   g [B][W][H][C] (the tape's input gradient), z0 / delta (B, C, W, H), both updated in place:
 *   rho_b = (float)(scale / max(sqrt(L[b]), 1e-8)) evaluated in fp64 on the device (L NULL: rho = 1);  t = g * inv_sf;  u = rho_b * t;
 *   z0 = z0 - u;  delta = delta + u.
 * _correct:  out = z_plain - p with p = c * delta, and z_plain's own bits where p is a zero of either sign. */
int rldm_guide_residual(const float* xhat, const float* y, const float* m, const float* wc, int B, int C, int W, int H, float* gx,
                        double* L, void* stream);
int rldm_guide_latent(const float* z0, float inv_sf, int B, int C, int W, int H, float* zin, void* stream);
int rldm_guide_update(const float* g, const double* L, double scale, float inv_sf, int B, int C, int W, int H, float* z0, float* delta,
                      void* stream);
int rldm_guide_correct(const float* z_plain, const float* delta, float c, int64_t n, float* out, void* stream);
int rldm_train_sqnorm(const float* g, int64_t n, double* out /*device*/, void* stream);
typedef struct rldm_adamw_config {
    float lr, beta1, beta2, eps, weight_decay;  /* torch.optim.AdamW, ldm/train_unconditional.py:357-363           */
    float max_grad_norm;                        /* clip_grad_norm_ (:548); <= 0: off; uses *sqnorm                 */
    float ema_decay;                            /* EMAModel.step (:556); used when ema != NULL                     */
    int32_t step;                               /* 1-based optimizer step (bias corrections)                       */
} rldm_adamw_config;
int rldm_train_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, const double* sqnorm,
                     int64_t n, const rldm_adamw_config* c, void* stream);
/* The same step with its per-step scalars read from device memory -- dyn[4] = (lr, 1 - beta1^step, 1 - beta2^step, ema decay),
 * written by rldm_train_hyper_step -- so a captured step graph can be replayed; zero_grads != 0 also clears `grads`
 * (optimizer.zero_grad(), ldm/train_unconditional.py:551). c->lr / c->step / c->ema_decay are ignored. */
int rldm_train_adamw_dyn(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* ema, const double* sqnorm,
                         int64_t n, const rldm_adamw_config* c, const float* dyn, int zero_grads, void* stream);
typedef struct rldm_hyper_config {
    float lr, beta1, beta2;                     /* base learning rate, AdamW betas                                  */
    float ema_max_decay, ema_inv_gamma, ema_power; /* EMAModel(use_ema_warmup=True) (:320-329)                      */
    int64_t lr_warmup_steps, total_steps;       /* get_scheduler("cosine", ...) (:394-399)                          */
} rldm_hyper_config;
/* step = ++*step_counter (device int64); dyn[4] <- the scalars of optimizer step `step` (lr of step - 1 scheduler steps). */
int rldm_train_hyper_step(int64_t* step_counter, const rldm_hyper_config* c, float* dyn, void* stream);
/* master fp32 [N][Cin][taps] -> bf16 [N][taps][ceil16(Cin)] (forward) and bf16 [Cin][taps][ceil16(N)] (flipped / transposed:
 * data gradient; may be NULL).  taps: 1, 9, or 16 (the discriminator's 4x4 convs, tap t = 4 i + j). */
int rldm_train_pack_weights(const float* w, int N, int Cin, int taps, void* w_forward, void* w_transposed, void* stream);
/* the same for every layer of the model in one launch: descs = DEVICE array sorted by `first` (cumulative count of
 * max(forward, transposed) copy elements), params = the flat fp32 parameter buffer. */
typedef struct rldm_pack_desc {
    int64_t first;          /* cumulative element index of this layer in the launch                               */
    int64_t param_offset;   /* offset of the layer's [N][Cin][taps] weight in the flat parameter buffer (elements) */
    void* w_forward;        /* bf16 [N][taps][ceil16(Cin)]                                                         */
    void* w_transposed;     /* bf16 [Cin][taps][ceil16(N)] or NULL                                                 */
    int32_t N, Cin, taps, pad_;
} rldm_pack_desc;
int rldm_train_pack_weights_all(const float* params, const rldm_pack_desc* descs, int num_layers, int64_t total, void* stream);
/* the same as a tiled transpose (coalesced reads and writes): descs[i].first = cumulative count of 64 x 64 (N, Cin) tiles,
 * total_tiles = their sum = the grid. */
int rldm_train_pack_weights_tiled(const float* params, const rldm_pack_desc* descs, int num_layers, int64_t total_tiles, void* stream);

/* ---- PatchGAN discriminator (rangeldm_amd/csrc/train_disc.hip; vae/sgm/modules/autoencoding/lpips/model/model.py:18-89,
 * NLayerDiscriminator, and losses/__init__.py, GeneralLPIPSWithDiscriminator after disc_start) ----
 * Driven by rangeldm_amd/discriminator.py.  Tensors as above: device fp32, NHWC [B][W][H][C], GEMM operands rounded to bf16 into the
 * MFMA with fp32 accumulation.  Scratch is the caller's: an entry point that needs some takes a workspace and says how large.
 *
 * 4x4 convolution with ZERO padding 1 ON BOTH AXES, stride 1 or 2.  W DOES NOT WRAP HERE, unlike every other conv of this library
 * (a range image is a cylinder, but the reference's discriminator is a plain nn.Conv2d(padding=1)): output (wo, ho) under tap
 * (i, j) in {0..3}^2 reads input (s wo + i - 1, s ho + j - 1), anything outside the tensor is zero.  Output size per axis:
 * (n + 2 - 4) / s + 1 (integer division; odd extents are legal at stride 2: 7 -> 3).  The desc describes the FORWARD conv in all
 * three directions.  Instances: Cin = 2 or a multiple of 16; N = 1 or a multiple of 16; Win, Hin >= 2; anything else is an error
 * (_ok: 0).  All of them run the same bf16 MFMA kernels (32x32x16), the boundary layers 2 -> 64 and 512 -> 1 on partly empty tiles. */
typedef struct rldm_train_disc_conv_desc {
    int32_t B, Win, Hin, Cin;   /* input tensor of the forward conv */
    int32_t N;                  /* output channels                  */
    int32_t stride;             /* 1 | 2                            */
} rldm_train_disc_conv_desc;
int rldm_train_disc_conv_ok(const rldm_train_disc_conv_desc* d);
/* y [B][Wo][Ho][N] = conv(x) + bias (bias may be NULL); w_packed = bf16 [N][16][ceil16(Cin)], tap t = 4 i + j, from
 * rldm_train_pack_weights(taps = 16). */
int rldm_train_disc_conv(const rldm_train_disc_conv_desc* d, const float* x, const void* w_packed, const float* bias, float* y,
                         void* stream);
/* dx [B][Win][Hin][Cin] = the data gradient for dy [B][Wo][Ho][N]; w_transposed = bf16 [Cin][16][ceil16(N)], taps flipped, from the
 * same call.  Stride 2: the four output parities (wi & 1, hi & 1) are four 2x2 convolutions over dy (the sub-pixel form), one grid
 * plane each; no tap that falls between the samples is multiplied. */
int rldm_train_disc_conv_dgrad(const rldm_train_disc_conv_desc* d, const float* dy, const void* w_transposed, float* dx, void* stream);
/* dw (N, Cin, 4, 4) torch layout += sum over pixels of dy (x) x (dw zeroed by the caller, as rldm_train_wgrad); dbias[N] += the
 * column sums of dy (NULL: none; rldm_train_colsum's arithmetic).  The pixels are cut into K slices whose partial tiles go to the
 * workspace and are added in slice order (from +0, then onto dw) IN BOTH MODES: no atomics reach dw.  _workspace: bytes needed. */
int64_t rldm_train_disc_wgrad_workspace(const rldm_train_disc_conv_desc* d);
int rldm_train_disc_wgrad(const rldm_train_disc_conv_desc* d, const float* dy, const float* x, float* dw, float* dbias,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* BatchNorm2d + LeakyReLU(0.2) over x [M][C] (M = B W H values per channel), eps 1e-5, momentum 0.1.
 *   training != 0: mean and BIASED variance per channel from fp64 sums (partial s covers rows [256 s, 256 s + 256): four lanes add
 *     rows s0 + k, s0 + k + 4, ... in order and meet k = 0 .. 3; the partials are added in order of s: fixed order in both modes);
 *     running_mean = 0.9 running_mean + 0.1 mean, running_var = 0.9 running_var + 0.1 var M / (M - 1) (the UNBIASED variance), both
 *     evaluated in fp64 and rounded once; *num_batches_tracked (device int64) += 1.  M < 2 is an error, as in torch.
 *   training == 0: mean = running_mean, var = running_var; nothing is updated.
 *   save [2 C] = (mean[C] | rstd[C]) fp32, rstd = the fp32 rounding of 1 / sqrt(var + 1e-5) in fp64: written in both cases, read by
 *     the backward.
 *   xhat = (x - mean) rstd;  z = xhat gamma + beta;  y = z > 0 ? z : 0.2 z     (fp32, every operation rounded on its own)
 * LeakyReLU's gradient at z == 0 is the slope-0.2 side (z <= 0), as torch's leaky_relu_backward (x > 0 ? dy : 0.2 dy).
 * _backward (training-mode statistics): dz = dy (z > 0 ? 1 : 0.2);  dbeta[c] += S1 = sum dz;  dgamma[c] += S2 = sum dz xhat (fp64
 *   sums, the forward's order);  dx = (gamma rstd) (dz - S1 / M - xhat S2 / M).  dgamma / dbeta may be NULL (input gradient only).
 * workspace: rldm_train_disc_bn_workspace(M, C) bytes. */
int64_t rldm_train_disc_bn_workspace(int64_t M, int C);
int rldm_train_disc_bn_forward(const float* x, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, int training, float* save, float* y,
                               void* workspace, int64_t workspace_bytes, void* stream);
int rldm_train_disc_bn_backward(const float* x, const float* dy, const float* save, int64_t M, int C, const float* gamma,
                                const float* beta, float* dx, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                                void* stream);
/* LeakyReLU(0.2) on its own (behind the first conv): backward == 0: y = x > 0 ? x : 0.2 x (dy unused);  backward != 0:
 * y = dy (x > 0 ? 1 : 0.2), the slope-0.2 side at x == 0. */
int rldm_train_disc_lrelu(const float* x, const float* dy, float* y, int64_t n, int backward, void* stream);
/* vqperceptual.hinge_d_loss times `factor`, over n logits each:  out (device double [3]) = (factor 0.5 (mean relu(1 - real) + mean
 * relu(1 + fake)), mean real, mean fake);  dreal = -g [1 - real > 0], dfake = +g [1 + fake > 0], g = factor 0.5 / n rounded once to
 * fp32 (1 - real and 1 + fake are the fp32 expressions).  Sums as rldm_train_l1: element 256 i + t is lane t of partial i, a
 * partial's 256 fp64 values meet in mse's binary tree, the partials in fp64 atomics -- or, in the deterministic mode, go to
 * partials [3][ceil(n / 256)] (device doubles, the caller's; may be NULL otherwise) and are folded as mse's.  No host sync. */
int rldm_train_disc_hinge(const float* real, const float* fake, int64_t n, float factor, float* dreal, float* dfake, double* out,
                          double* partials, void* stream);
/* The generator term: *out (device double) = -mean(fake), dfake = -1 / n (rounded once to fp32); sums and partials [ceil(n / 256)]
 * as above. */
int rldm_train_disc_generator(const float* fake, int64_t n, float* dfake, double* out, double* partials, void* stream);
/* The adaptive weight and the gradient mix in one element-wise launch that reads the squared norms from device memory:
 *   d_weight = clamp(sqrt(*sq_nll) / (sqrt(*sq_g) + 1e-4), 0, 1e4) disc_weight   (fp64; written to *d_weight, a device double)
 *   dpred[i] = dnll[i] + s dg[i],  s = d_weight disc_factor rounded once to fp32; product and sum rounded on their own. */
int rldm_train_disc_adaptive_mix(const float* dnll, const float* dg, const double* sq_nll, const double* sq_g, float disc_weight,
                                 float disc_factor, float* dpred, double* d_weight, int64_t n, void* stream);

/* ---- Meta-Kernel discriminator layer (rangeldm_amd/csrc/train_meta.hip; model.py:91-265, MetaKernel and
 * NLayerDiscriminatorMetaKernel, which vae/configs/kitti360.yaml selects) ----
 * Driven by rangeldm_amd/metakernel.py.  One layer: a 4x4 window, padding 1, stride 1 | 2, over x [B][W][H][C] and the range image
 * r [B][W][H].  For output pixel (wo, ho) and tap t = 4 i + j (i: shift along H, j: shift along W) the source is w = (s wo + j - 1)
 * mod W (W WRAPS), h = s ho + i - 1; outside [0, H) x reads 0 and r reads 100.  Wo = (W - 2) / s + 1, Ho = (H - 2) / s + 1.  A ROW
 * is a (pixel, tap) pair, row = 16 px + t.  In fp32, in this order, with tables [4][16] = cos_azi | sin_azi | cos_inc | sin_inc:
 *   rc = r[(s wo + 1) mod W][s ho + 1];  pe0 = (rt ca[t]) ci[t] - rc;  pe1 = (rt ca[t]) si[t];  pe2 = rt sa[t]
 *   h[k] = lrelu_0.2(((W1[k][0] pe0 + W1[k][1] pe1) + W1[k][2] pe2) + b1[k])
 *   m[c] = sum_k r(h[k]) r(W2[c][k]) + b2[c]           (bf16 MFMA, fp32 accumulation; C = 2: fp32 on the VALU, nothing rounded)
 *   y[n] = sum_{t,c} r(m[c] x[c]) r(coov[n][16 c + t]) + bias[n]    (bf16 MFMA);   r_next[px] = rc
 * r(.) rounds to bf16 as the operand tile is staged in LDS.  Kept for the backward, the caller's: pe [rows][3], src [rows] (the
 * source pixel index, -1 outside H), m [rows][C] fp32.  Backward, from dy [B][Wo][Ho][N]:
 *   G = r(dy) r(coov);  dcoov += r(dy)^T r(m x);  dbias += colsum dy;  dx = gather of G m;  dm = G x;  db2 += colsum dm;
 *   dW2 += r(dm)^T r(h);  dh = r(dm) r(W2);  dpre = dh lrelu'(pre);  db1 += colsum dpre;  dW1 += dpre^T pe and dpe = dpre W1 in fp32;
 *   dr = gather of dpe over both roles of a pixel (tap: (dpe0 ci) ca + (dpe1 si) ca + dpe2 sa; centre: minus its pixel's sixteen
 *   dpe0) + dr_next of the pixel whose centre it is.
 * Gathers, not scatters: no floating-point atomics; split reductions leave partial tiles that are added in slice order in both modes
 * of rldm_train_deterministic (the three column sums are rldm_train_colsum's).  The six parameter gradients (into zeroed or
 * accumulating buffers) are given together or all NULL (input gradient alone); dx may be NULL (no data gradient), dr NULL with or
 * without it (no range gradient: a discriminator step never needs one).
 * Instances: C = 2 or a multiple of 16; N = 1 or a multiple of 16; stride 1 | 2; W, H >= 2; anything else is an error (_ok: 0). */
typedef struct rldm_train_meta_desc {
    int32_t B, Win, Hin, C;     /* input tensor */
    int32_t N;                  /* output channels */
    int32_t stride;             /* 1 | 2 */
} rldm_train_meta_desc;
int rldm_train_meta_ok(const rldm_train_meta_desc* d);
/* bytes of scratch for _forward / _backward */
int64_t rldm_train_meta_workspace(const rldm_train_meta_desc* d);
/* r[p] = (x[p][0] range_std + range_mean) / 10 over npix pixels of C channels; _range_grad: dx[p][0] += (dr[p] / 10) range_std */
int rldm_train_meta_range(const float* x, int64_t npix, int C, float range_mean, float range_std, float* r, void* stream);
int rldm_train_meta_range_grad(const float* dr, int64_t npix, int C, float range_std, float* dx, void* stream);
int rldm_train_meta_forward(const rldm_train_meta_desc* d, const float* x, const float* r, const float* tables, const float* w1,
                            const float* b1, const float* w2, const float* b2, const float* coov, const float* bias, float* y,
                            float* r_next, float* pe, int32_t* src, float* m, void* workspace, int64_t workspace_bytes, void* stream);
int rldm_train_meta_backward(const rldm_train_meta_desc* d, const float* x, const float* dy, const float* tables, const float* w1,
                             const float* b1, const float* w2, const float* coov, const float* pe, const int32_t* src, const float* m,
                             const float* dr_next, float* dx, float* dr, float* dw1, float* db1, float* dw2, float* db2, float* dcoov,
                             float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- introspection used by bench.py / tests ----------------------------------------------------------------- */
/* algorithmic FLOPs (2*MACs of conv/linear/QK^T/PV) of one UNet forward / VAE decode / encode for batch B */
double rldm_unet_flops(rldm_unet* m, int B);
double rldm_vae_decode_flops(rldm_vae* m, int B, int latent_w, int latent_h);
/* number of kernel launches in one UNet forward plan (for the launch-overhead budget in DESIGN.md) */
int rldm_unet_num_launches(rldm_unet* m, int B);

/* Instrumented pass used by bench.py for the roofline: runs ONE UNet step (+ one VAE decode) eagerly on the sampler's
 * stream with a HIP event pair around every kernel launch and writes JSON
 *   {"unet_step": {kernel: {launches, ms, flops, bytes}, ...}, "vae_decode": {...}, "plan_flags": F, "fell_back": bool, ...}
 * (flops/bytes = algorithmic work of those launches; plan_flags = the routing bits in effect for this sampler's plans,
 * fell_back = the library added bits of its own, i.e. a persistent launch failed its self-check earlier) into json_out. */
int rldm_sampler_profile(rldm_sampler* s, const float* x_T, char* json_out, size_t cap);

/* low-level op entry points (used by the parity tests to check each kernel in isolation) */
typedef struct rldm_conv_desc {
    int32_t B, Cin0, Cin1, Win, Hin;  /* inputs x0 [B][Win][Hin][Cin0] (+ x1 [..][Cin1] concatenated), bf16 NHWC */
    int32_t Cout;
    int32_t ksize;                    /* 1 or 3                                                                */
    int32_t stride;                   /* 1 or 2                                                                */
    int32_t pad_mode;                 /* 0: symmetric pad 1 (wrap W / zero H); 1: end-only pad (VAE downsample) */
    int32_t upsample;                 /* 1: nearest x2 folded into the input indexing                          */
    int32_t gn;                       /* 1: GroupNorm(32) prologue on the (concatenated) input                  */
    int32_t silu;                     /* 1: SiLU after the norm                                                */
    float eps;
} rldm_conv_desc;
/* One fused conv: y = conv(silu(GN(cat[x0,x1]))) + bias + temb[b] + res.  All device pointers; x0/x1/res/y are
 * fp32 NCHW here (converted on device) so tests can feed reference tensors; weight (Cout, Cin, k, k), gamma/beta,
 * bias, temb ([B][Cout] or NULL) are HOST fp32. */
int rldm_test_conv(const rldm_conv_desc* d, const float* x0, const float* x1, const float* weight, const float* bias,
                   const float* gamma, const float* beta, const float* temb, const float* res, float* y, void* stream);
/* kernel-tuning aids (tools/bench_conv.py): time the fused conv kernel alone on synthetic data with HIP events on
 * `stream` (avg_us per launch over `iters` back-to-back launches; with_res = channels of the fused residual phase:
 * 0 none, Cout identity, else a synthetic 1x1 shortcut); force the pixel/channel tile and split-K (0 = automatic). */
int rldm_bench_conv(const rldm_conv_desc* d, int with_res, int with_temb, int warmup, int iters, float* avg_us,
                    char* kernel_name, size_t name_cap, void* stream);
int rldm_debug_force_tile(int BM, int BN, int ksplit);
/* self-check word of the persistent trunk launches (trunk.hip) of the batch-B plan of a UNet: 0 fine or no trunk, 1 a bounded
 * wait gave up, 2 a cluster of workgroups was spread over several XCDs; synchronises the device */
int rldm_unet_trunk_status(rldm_unet* m, int B);
/* routing options of the rldm_unet_forward plans of ONE model (the bits of rldm_debug_set_flags, scoped; drops its cached plans) */
int rldm_unet_set_plan_flags(rldm_unet* m, int flags);
/* tests: the next rldm_sample of `s` behaves as if a cluster wait had given up in the middle of the run (code 1 or 2) */
int rldm_debug_inject_trunk_error(rldm_sampler* s, int code);
int rldm_debug_timestamps(unsigned long long* host_out);   /* NULL: enable; else read back [4][64] s_memtime stamps */
int rldm_debug_block_times(unsigned long long* host_out, int nblocks);   /* ABLATE builds: [start, end] (100 MHz) of every workgroup of the last conv_stream launch */
/* Routing switches, PROCESS-WIDE, read when a plan is built (RLDM_DBG_FLAGS seeds the first word): for tests and tuning runs.  A host
 * that wants one sampler / model routed differently uses rldm_sampler_config::plan_flags / rldm_unet_set_plan_flags (the same
 * RLDM_FLAG_* bits, scoped), and the library's own fall-backs are scoped the same way.  0 restores the defaults.  The switches
 * choose the launches of a plan; they do not reach the kernels (only the -DRLDM_ABLATE timeline build hands the word on). */
enum rldm_flag {
    RLDM_FLAG_ATTN_PROJ_LAUNCH = 1 << 7,    /* the attention output projection as a launch of its own                              */
    RLDM_FLAG_NO_CONV_SMALL    = 1 << 8,    /* no conv_small route                                                                  */
    RLDM_FLAG_SMALL_128PX      = 1 << 10,   /* the 128x8 level on conv_small's 128-pixel tiles                                      */
    RLDM_FLAG_NO_STREAM_REGW   = 1 << 11,   /* no conv_stream / conv_c16 / conv_o4 / conv_ds2 / conv_regw route (with
                                             * RLDM_FLAG_NO_CONV_SMALL: every conv on the generic kernel)                           */
    RLDM_FLAG_STREAM_ANY_GRID  = 1 << 12,   /* conv_stream wherever it fits, whatever its grid size                                 */
    RLDM_FLAG_GRAPH_TRACE      = 1 << 13,   /* stamps between the launches of a sampler's step graph (rldm_debug_graph_trace)       */
    RLDM_FLAG_SMALL_64PX_32X2  = 1 << 19,   /* 32x2 images as one 64-pixel conv_small tile (default: two 32-pixel tiles)            */
    RLDM_FLAG_CONSUMER_GN      = 1 << 20,   /* every GroupNorm applied by its consumer (no producer-side normalised copies)         */
    RLDM_FLAG_NO_WIDE_SPLIT    = 1 << 21,   /* concatenations over 512 channels on the generic kernel, not run half by half         */
    RLDM_FLAG_OWN_IMAGE_COPIES = 1 << 22,   /* every conv that can own its image does, and writes two normalised copies (tests)     */
    RLDM_FLAG_SCHED_LAUNCH     = 1 << 23,   /* the sampler's scheduler step as launches of their own                                */
    RLDM_FLAG_NO_PERSISTENT    = 1 << 24,   /* no persistent launches: every layer a launch of its own, same tiles, same results    */
    RLDM_FLAG_NO_CLUSTERS      = 1 << 26    /* no multi-tile clusters (the 64x4 / 256x16 levels as launches: for a shared GPU)      */
};
int rldm_debug_set_flags(int flags);
/* second word of the same kind (no environment seed) */
enum rldm_flag2 {
    RLDM_FLAG2_STREAM_8WAVE_FULL = 1,       /* full-resolution conv_stream launches keep the 8-wave 256-pixel workgroups            */
    RLDM_FLAG2_STREAM_8WAVE_128X8 = 2,      /* the 128x8 level keeps the 8-wave 128 x 64 x 4-k-group workgroups                     */
    RLDM_FLAG2_STREAM_8WAVE_C64 = 4,        /* the VAE's 64-channel level keeps the 8-wave 256 x 64 workgroups                      */
    RLDM_FLAG2_STREAM_SPEC_WAVES = 32,      /* the 256 x 128 conv_stream tile with specialised matrix / staging waves              */
    RLDM_FLAG2_STREAM_64PX = 64,            /* the 8 x 8 x 128-channel x 2-k-group conv_stream tile wherever it fits                */
    RLDM_FLAG2_NO_REGW = 1 << 24,           /* the VAE decoder's 64 -> 64 convs and conv_out on the per-tile kernels, not conv_regw  */
    RLDM_FLAG2_REGW_CAP8 = 1 << 25,         /* conv_regw's grid capped at 8 runs (runs of several tiles on small test images)      */
    RLDM_FLAG2_FP32_OUT = 1 << 26,          /* a test / bench conv of <= 4 output channels is an fp32-NCHW output layer            */
    RLDM_FLAG2_HALO_RING = 1 << 29          /* 16 x 8 conv_stream tiles with a staged halo ring at the 16- / 8-beam levels          */
};
int rldm_debug_set_flags2(int flags);
/* in-graph timeline of the UNet ops of the sampler's step graph (RLDM_FLAG_GRAPH_TRACE set before rldm_sampler_create) */
int rldm_debug_graph_trace(unsigned long long* stamps, int cap, char* names, size_t names_cap);
/* statistics side-output of the conv epilogue (feeds the next GroupNorm): stats device fp32 [B][Cout][2] = per-image
 * (sum, sum of squares) of the bf16 outputs of conv(x0); plain single-input conv only. */
int rldm_test_conv_stats(const rldm_conv_desc* d, const float* x0, const float* weight, const float* bias, float* stats,
                         void* stream);
/* (tests) the scheduler step where a captured sampler runs it: in the epilogue of the UNet's output layer.  The conv of `d` (Cout <= 4,
 * no x1) is built as an output layer -- fp32 NCHW, whatever RLDM_FLAG2_FP32_OUT says -- and run once with the plan's scheduler block
 * filled from `sch`, exactly the fields a sampler fills: the mode word comes from the function the sampler uses.  All pointers of
 * the struct are device pointers.  The launch reads row *step of coef_table and, when that row's coef[4] != 0, the noise at
 * noise + *step * noise_step_stride; RLDM_SAMPLER_DPMSOLVER: `noise` is the x0 history (stride 0), read under the same rule and
 * then overwritten with this step's x0.  x, noise, x_prev: fp32 [B][Cout][W][H]; x_prev may alias x.  pack (or NULL): the next
 * step's conv_in input, bf16 [B][W][H][pack_ld], of which channels < Cout receive bf16(x_prev). */
typedef struct rldm_conv_sched_desc {
    int32_t sampler_mode;             /* RLDM_SAMPLER_*                                                        */
    int32_t prediction_type;          /* RLDM_PRED_*                                                           */
    const float* coef_table;          /* [rows][5]                                                             */
    const int32_t* step;
    const float* x;
    const float* noise;
    int64_t noise_step_stride;
    float* x_prev;
    void* pack;
    int32_t pack_ld;
} rldm_conv_sched_desc;
/* x0 device fp32 NCHW; weight, bias, gamma, beta HOST fp32 as in rldm_test_conv; eps: device fp32 [B][Cout][W][H], the conv's own
 * output.  op_name receives the name of the launch that carried the step (e.g. "conv_o4_kernel<128,32,taps9>"). */
int rldm_test_conv_sched(const rldm_conv_desc* d, const float* x0, const float* weight, const float* bias, const float* gamma,
                         const float* beta, const rldm_conv_sched_desc* sch, float* eps, char* op_name, size_t name_cap, void* stream);
/* (tests) the time-embedding table on its own: n timesteps (host), converted as rldm_unet_forward converts them, through the model's
 * Timesteps -> TimestepEmbedding -> every resnet's time_emb_proj(SiLU(emb)) launches -> table device fp32 [n][ld].  The model needs
 * to be finalized only; any n >= 1 (a forward takes 1 or B rows, a sampler num_steps). */
int rldm_test_temb(rldm_unet* m, const int64_t* timesteps, int n, float* table, void* stream);
/* (tests) the table's layout: resnet_prefix NULL -> *value = ld, the row length; else (e.g. "down_blocks.0.resnets.1") the column
 * at which that resnet's projection starts (its out_channels columns follow).  Fails on a prefix the model does not have. */
int rldm_test_temb_layout(rldm_unet* m, const char* resnet_prefix, int* value);
/* multi-head (d=8) self-attention core: qkv device fp32 [B][L][3C] -> out device fp32 [B][L][C] */
int rldm_test_attention(const float* qkv, int B, int L, int C, float* out, void* stream);
/* the launch every attention block of the UNet actually runs -- GroupNorm -> to_q / to_k / to_v -> softmax(q k^T/sqrt 8) v
 * (diffusers Attention before to_out; reference analogue vae/sgm/modules/attention.py:194-284 behind a GroupNorm):
 * x device fp32 [B][L][C] token-major, gamma / beta host [C], wqkv host [3C][C] (q | k | v rows), bqkv host [3C]
 * -> out device fp32 [B][L][C], heads concatenated. */
int rldm_test_attention_qkv(const float* x, int B, int L, int C, int groups, float eps, const float* gamma, const float* beta,
                            const float* wqkv, const float* bqkv, float* out, void* stream);
/* (tests) what that launch runs for (B, L, C): route[0] = 2 (attention_qkv2_d8_kernel) or 1 (the first generation,
 * attention_qkv_d8_kernel), [1] PAIR (two query tiles per wave), [2] HG (heads per workgroup), [3] waves per workgroup,
 * [4] 1 if the output projection can ride on the launch for the shape alone, [5] ... and on this device's CU count (the seam). */
int rldm_test_attention_route(int B, int L, int C, int* route);
/* (tests) the whole block: that launch, then y = x + to_out(o) with to_out_w host [C][C], to_out_b host [C]; mode 0: the output
 * projection as a launch of its own, 1: behind the seam inside the launch (fails if the device cannot hold every workgroup at
 * once, or if the seam reports an error), 2: the regular 1x1 conv of the unfused plan.  Needs a shape whose launch can carry the
 * projection (route[4]).  y device fp32 [B][L][C] (the bf16 output); stats device fp32 [B][L/64][C][2] = the (sum, sum of squares)
 * partials of y per 64-token block (mode 2: the per-image totals of the conv's partials in block 0, the other blocks zero). */
int rldm_test_attention_block(const float* x, int B, int L, int C, int groups, float eps, const float* gamma, const float* beta,
                              const float* wqkv, const float* bqkv, const float* to_out_w, const float* to_out_b, int mode, float* y,
                              float* stats, void* stream);
/* HIP-event time of that launch alone on synthetic data (tools/bench_attn.py) */
int rldm_bench_attention_qkv(int B, int L, int C, int warmup, int iters, float* avg_us, void* stream);

/* ---- calibration of the box (bench.py `calibration`; the metric's definition) -----------------------------------
 * What this GPU does right now, measured in the benchmark's own process so that a throughput line can be read against it:
 * mfma_tflops / mfma_clock_mhz = a pure v_mfma_f32_32x32x16_bf16 loop on every SIMD (HIP events) and the shader clock while it runs
 * (s_memtime ticks per s_memrealtime tick x 100 MHz); copy_gbs = a 1 GiB device-to-device copy, bytes read + written per second.
 * Synchronises the stream; allocates and frees 2 GiB. */
int rldm_calibrate(double* mfma_tflops, double* mfma_clock_mhz, double* copy_gbs, void* stream);
/* Clock stamps around any work on `stream`: RLDM_CALIB_STAMP_BLOCKS workgroups (block ids go round the XCDs) each write
 * slots[4 * block + {0, 1, 2, 3}] = {XCC id, s_memtime, s_memrealtime, 1}.  Two stamps of the same XCC id: (d s_memtime / d s_memrealtime)
 * x 100 MHz = the mean shader clock over what ran between them.  slots: device, 4 * RLDM_CALIB_STAMP_BLOCKS uint64. */
#define RLDM_CALIB_STAMP_BLOCKS 16
int rldm_calib_clock_stamp(unsigned long long* slots, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RANGELDM_HIP_H */
