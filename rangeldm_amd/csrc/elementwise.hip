// Small HBM-bound kernels of the RangeLDM path (gfx950): boundary layout conversions, conv_in input packing
// (pos-encoding channel / per-step condition concat without a `torch.cat` copy), timestep embedding + all per-resnet
// projections in one launch, DDIM / DDPM scheduler steps, add_noise, DiagonalGaussian sampling.
#include "kernels.h"

namespace rldm {

// ---- conv_in input: [B][W][H][Cpad] bf16 <- x (cx ch, fp32 NCHW, * scale) | pos-encoding | cond (cc ch) | 0 --------
// replaces torch.cat([latents, pos_encoding], 1) / torch.cat([latents, image], 1): ldm/pipelines.py:238,358,498
__global__ void __launch_bounds__(256) pack_input_kernel(const PackInputParams p) {
    const long long npix = (long long)p.B * p.W * p.H;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    // the sampler's step index: advanced by the first launch of a step (nothing in this kernel reads it; every later launch of the
    // step sees the new value across the kernel boundary) instead of by a one-thread launch of its own behind the scheduler step
    if (i == 0 && p.step_inc) *p.step_inc += 1;
    if (i >= npix) return;
    const int hw = p.W * p.H;
    const int b = (int)(i / hw);
    const int r = (int)(i - (long long)b * hw);
    const int w = r / p.H;
    bf16_t* dst = p.out + i * p.Cpad;
    int c = 0;
    for (int k = 0; k < p.cx; ++k, ++c) dst[c] = f32_to_bf16(p.x[((size_t)b * p.cx + k) * hw + r] * p.scale);
    if (p.pos_encoding) dst[c++] = f32_to_bf16(w == 0 ? 1.0f : 0.0f);
    for (int k = 0; k < p.cc; ++k, ++c) dst[c] = f32_to_bf16(p.cond[((size_t)b * p.cc + k) * hw + r]);
    for (; c < p.Cpad; ++c) dst[c] = 0;
}

int launch_pack_input(const PackInputParams& p, hipStream_t stream) {
    RLDM_REQUIRE(p.cx + (p.pos_encoding ? 1 : 0) + p.cc <= p.Cpad, "pack_input: channels exceed padded width");
    const long long npix = (long long)p.B * p.W * p.H;
    hipLaunchKernelGGL(pack_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* src, bf16_t* dst, int B, int C, int hw, int Cpad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over B*hw*Cpad, c fastest
    const long long total = (long long)B * hw * Cpad;
    if (i >= total) return;
    const int c = (int)(i % Cpad);
    const long long pix = i / Cpad;
    const int b = (int)(pix / hw), r = (int)(pix - (long long)b * hw);
    dst[i] = c < C ? f32_to_bf16(src[((size_t)b * C + c) * hw + r]) : (bf16_t)0;
}
int launch_nchw_f32_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, int W, int H, int Cpad, hipStream_t s) {
    const long long total = (long long)B * W * H * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, B, C,
                       W * H, Cpad);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const bf16_t* src, float* dst, int B, int C, int hw, int ld) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over B*C*hw, r fastest
    const long long total = (long long)B * C * hw;
    if (i >= total) return;
    const int r = (int)(i % hw);
    const long long bc = i / hw;
    const int c = (int)(bc % C), b = (int)(bc / C);
    dst[i] = bf16_to_f32(src[((size_t)b * hw + r) * ld + c]);
}
int launch_nhwc_bf16_to_nchw_f32(const bf16_t* src, float* dst, int B, int C, int W, int H, int ld, hipStream_t s) {
    const long long total = (long long)B * C * W * H;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, B, C,
                       W * H, ld);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- time embedding + every resnet's time_emb_proj ------------------------------------------------------------------
// diffusers Timesteps(flip_sin_to_cos, freq_shift) + TimestepEmbedding + ResnetBlock2D.time_emb_proj(SiLU(emb))
// [3P; SURVEY.md A.2]; analogue vae/sgm/modules/diffusionmodules/model.py:28-46,349.  fp32 throughout.
// Three launches of one row-batched Linear: out[r][o] = act(b[o] + sum_k w[o][k] * in[r][k]).  A workgroup owns 16
// outputs for ALL rows (its 16 weight rows are read once), lane = row, the K loop runs over 128-wide chunks staged in
// LDS (pitch 132 floats: 16-byte reads of 8 consecutive lanes cover the 32 banks), weights are LDS broadcasts.
// The [50][4352] table of a 50-step sampler is 272 + 32 + 32 workgroups instead of 50 (3.3 ms -> tens of us).
constexpr int TL_OB = 16, TL_KC = 128, TL_PITCH = TL_KC + 4;
struct RowsLinearParams {
    const float* in;        // [rows][K], or null: the sinusoid of t
    const float* t;         // [rows] (sinusoid mode)
    int flip, shift;
    const float* w; const float* b;   // [O][K], [O]
    float* out; int ldo;
    int rows, K, O, act;
};
__global__ void __launch_bounds__(256) rows_linear_kernel(const RowsLinearParams p) {
    __shared__ float xs[64 * TL_PITCH];
    __shared__ float ws[TL_OB * TL_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * TL_OB;
    const int half = p.K / 2;
    for (int r0 = 0; r0 < p.rows; r0 += 64) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < p.K; kc += TL_KC) {
            __syncthreads();
            for (int i = tid; i < 64 * TL_KC; i += 256) {
                const int r = i / TL_KC, k = i % TL_KC, kk = kc + k;
                float v = 0.f;
                if (r0 + r < p.rows && kk < p.K) {
                    if (p.in) v = p.in[(size_t)(r0 + r) * p.K + kk];
                    else {
                        const int j = kk % half;
                        const float f = expf(-9.210340371976184f * (float)j / (float)(half - p.shift));   // ln(10000)
                        const float a = p.t[r0 + r] * f;
                        const bool first = kk < half;
                        v = (first == (p.flip != 0)) ? cosf(a) : sinf(a);      // [sin, cos]; halves swapped when flip
                    }
                }
                xs[r * TL_PITCH + k] = v;
            }
            for (int i = tid; i < TL_OB * TL_KC; i += 256) {
                const int o = i / TL_KC, k = i % TL_KC;
                ws[o * TL_PITCH + k] = (o0 + o < p.O && kc + k < p.K) ? p.w[(size_t)(o0 + o) * p.K + kc + k] : 0.f;
            }
            __syncthreads();
            const float4* xr = reinterpret_cast<const float4*>(xs + lane * TL_PITCH);
#pragma unroll 4
            for (int k4 = 0; k4 < TL_KC / 4; ++k4) {
                const float4 x = xr[k4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 w = reinterpret_cast<const float4*>(ws + (wave * 4 + j) * TL_PITCH)[k4];
                    acc[j] += w.x * x.x + w.y * x.y + w.z * x.z + w.w * x.w;
                }
            }
        }
        if (r0 + lane < p.rows) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = o0 + wave * 4 + j;
                if (o < p.O) {
                    float v = acc[j] + p.b[o];
                    if (p.act) v = silu_f(v);
                    p.out[(size_t)(r0 + lane) * p.ldo + o] = v;
                }
            }
        }
    }
}
int launch_temb(const TembParams& p, hipStream_t stream) {
    float* h1 = p.scratch;
    float* h2 = p.scratch + (size_t)p.rows * p.D;
    RowsLinearParams a{};
    a.in = nullptr; a.t = p.t; a.flip = p.flip_sin_to_cos; a.shift = p.freq_shift;
    a.w = p.w1; a.b = p.b1; a.out = h1; a.ldo = p.D; a.rows = p.rows; a.K = p.dim0; a.O = p.D; a.act = 1;
    hipLaunchKernelGGL(rows_linear_kernel, dim3((a.O + TL_OB - 1) / TL_OB), dim3(256), 0, stream, a);
    a.in = h1; a.w = p.w2; a.b = p.b2; a.out = h2; a.K = p.D;        // h2 = SiLU(emb): what every time_emb_proj reads
    hipLaunchKernelGGL(rows_linear_kernel, dim3((a.O + TL_OB - 1) / TL_OB), dim3(256), 0, stream, a);
    a.in = h2; a.w = p.wp; a.b = p.bp; a.out = p.out; a.ldo = p.total; a.O = p.total; a.act = 0;
    hipLaunchKernelGGL(rows_linear_kernel, dim3((a.O + TL_OB - 1) / TL_OB), dim3(256), 0, stream, a);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- scheduler steps (diffusers DDIMScheduler.step / DDPMScheduler.step [3P]; DPMSolverMultistepScheduler.step)
__global__ void __launch_bounds__(256) sched_step_kernel(const SchedParams p) {
    float c0, c1, c2, c3, c4;
    const float* nz = p.noise;
    if (p.coef_table) {
        const int step = *p.step_ptr;
        const float* c = p.coef_table + 5 * step;
        c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4];
        if (nz) nz += (size_t)step * p.noise_step_stride;
    } else {
        c0 = p.coef[0]; c1 = p.coef[1]; c2 = p.coef[2]; c3 = p.coef[3]; c4 = p.coef[4];
    }
    const bool use_noise = nz != nullptr && c4 != 0.f;
    float* const hist = sched_history(p.mode, p.noise);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long long)gridDim.x * 256) {
        const float x = p.x[i], e = p.eps[i];
        float x0;
        const float prev = sched_prev(p.mode, c0, c1, c2, c3, c4, x, e, use_noise ? nz[i] : 0.f, use_noise, x0);
        if (hist) hist[i] = x0;
        p.x_prev[i] = prev;
    }
}
int launch_sched_step(const SchedParams& p, hipStream_t stream) {
    RLDM_REQUIRE(p.mode >= 0, "scheduler step: this sampler mode has no 5-wide row (sched_mode_word)");
    const unsigned grid = (unsigned)((p.n + 255) / 256 > 2048 ? 2048 : (p.n + 255) / 256);
    hipLaunchKernelGGL(sched_step_kernel, dim3(grid), dim3(256), 0, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- guided scheduler step (RePaint-style known-region replacement on an unconditional sampler) -------------------------------
// Per element of the lane's sample, in fp32:  u = the scheduler step above (same expression, same row, same roundings);
//   g = m * (ka * z0 + kb * nk) + (1 - m) * u      m = the one-channel mask at sample resolution, broadcast over channels (1: known)
//   x' = ra * g + rb * nr                          (ra, rb) = (1, 0) on rows that do not jump back up
// Row = {c0 .. c4, ka, kb, ra, rb}.  m == 1 and m == 0 are SELECTIONS: a known pixel does not depend on u (an inf there stays
// there), an unknown one not on z0 / nk.  ka * z0 + kb * nk is two roundings of the products and one of the sum (no contraction),
// so a host can restate it bit for bit; nk is read only when kb != 0, nr only when the row jumps.
// u is sched_prev (kernels.h), whose roundings are stated there: this kernel and sched_step_kernel evaluate the same sequence
// (tests/test_guided_gpu.py holds the two bit-equal for every mode and prediction type).
__device__ __forceinline__ float guided_known(const float ka, const float z0, const float kb, const float nk, const bool use_nk) {
#pragma clang fp contract(off)
    const float a = ka * z0;
    if (!use_nk) return a;
    const float b = kb * nk;
    return a + b;
}
template <int V> struct GuidedVec { float v[V]; };
template <int V> __device__ __forceinline__ GuidedVec<V> guided_load(const float* p) {
    GuidedVec<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void guided_store(float* p, const GuidedVec<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}
// V = 4: n, spatial and every pointer (step strides included) are multiples of 4 floats -- the four elements of a group share
// their image and channel, so the mask is one float4 as well.  V = 1: any shape.
template <int V> __global__ void __launch_bounds__(256) sched_guided_step_kernel(const GuidedSchedParams p) {
    float c0, c1, c2, c3, c4, ka, kb, ra, rb;
    const float* nz = p.s.noise;
    const float* nk = p.known_noise;
    const float* nr = p.renoise_noise;
    if (p.s.coef_table) {
        const int step = *p.s.step_ptr;
        const float* c = p.s.coef_table + 9 * step;
        c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; ka = c[5]; kb = c[6]; ra = c[7]; rb = c[8];
        const size_t off = (size_t)step * p.s.noise_step_stride;
        if (nz) nz += off;
        if (nk) nk += off;
        if (nr) nr += off;
    } else {
        c0 = p.s.coef[0]; c1 = p.s.coef[1]; c2 = p.s.coef[2]; c3 = p.s.coef[3]; c4 = p.s.coef[4];
        ka = p.k[0]; kb = p.k[1]; ra = p.k[2]; rb = p.k[3];
    }
    const bool use_noise = nz != nullptr && c4 != 0.f;
    const bool use_nk = nk != nullptr && kb != 0.f;
    const bool jump = nr != nullptr && (ra != 1.f || rb != 0.f);
    const long long groups = p.s.n / V;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < groups; q += (long long)gridDim.x * 256) {
        const long long i = q * V;
        const long long mi = (i / p.per_sample) * p.spatial + i % p.spatial;
        const GuidedVec<V> x = guided_load<V>(p.s.x + i), e = guided_load<V>(p.s.eps + i);
        const GuidedVec<V> z0 = guided_load<V>(p.known + i), m = guided_load<V>(p.mask + mi);
        GuidedVec<V> zn, zk, zr, out;
        if (use_noise) zn = guided_load<V>(nz + i);
        if (use_nk) zk = guided_load<V>(nk + i);
        if (jump) zr = guided_load<V>(nr + i);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float x0;
            const float u = sched_prev(p.s.mode, c0, c1, c2, c3, c4, x.v[j], e.v[j], use_noise ? zn.v[j] : 0.f, use_noise, x0);
            const float kn = guided_known(ka, z0.v[j], kb, use_nk ? zk.v[j] : 0.f, use_nk);
            const float mm = m.v[j];
            float g = mm == 1.f ? kn : u;
            if (mm != 1.f && mm != 0.f) g = mm * kn + (1.f - mm) * u;
            if (jump) g = ra * g + rb * zr.v[j];
            out.v[j] = g;
        }
        guided_store<V>(p.s.x_prev + i, out);
    }
}
int launch_sched_guided_step(const GuidedSchedParams& p, hipStream_t stream) {
    RLDM_REQUIRE(p.s.mode >= 0, "guided scheduler step: this sampler mode has no 5-wide row (sched_mode_word)");
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = p.s.n % 4 == 0 && p.spatial % 4 == 0 && p.s.noise_step_stride % 4 == 0 && al(p.s.x) && al(p.s.eps) &&
                     al(p.s.x_prev) && al(p.s.noise) && al(p.known) && al(p.mask) && al(p.known_noise) && al(p.renoise_noise);
    const long long groups = vec ? p.s.n / 4 : p.s.n;
    const unsigned grid = (unsigned)((groups + 255) / 256 > 2048 ? 2048 : (groups + 255) / 256);
    if (vec) hipLaunchKernelGGL(sched_guided_step_kernel<4>, dim3(grid), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(sched_guided_step_kernel<1>, dim3(grid), dim3(256), 0, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- UniPC step (diffusers UniPCMultistepScheduler.step: bh2, predict_x0; include/rangeldm_hip.h, rldm_sched_unipc_step) --------------
// Per element, fp32, row c = {alpha, s, use_corr, k_last, k_1, k_2, k_3, k_t, p_x, p_0, p_1, p_2}, h0 / h1 / h2 = the x0 predictions of the
// three previous steps:
//   m   = x0 of the model output (the conversions of sched_prev, with the sample the network saw)
//   x_c = use_corr ? k_last * last + k_1 * h0 + k_2 * h1 + k_3 * h2 + k_t * m : x          (UniC, order of the previous step)
//   x'  = p_x * x_c + p_0 * m + p_1 * h0 + p_2 * h1                                         (UniP)
//   last <- x_c, h2 <- h1, h1 <- h0, h0 <- m       by the thread that read them: the step graph replays with the same pointers
// A term whose coefficient is 0 is left out, not multiplied: a first step runs on a history that holds anything (NaN included), and
// `last` / h2 are then not even loaded.  h0 and h1 are always loaded -- the shift moves them.
// Groups of four elements move as one 16-byte load or store per tensor (global_load_dwordx4 / global_store_dwordx4: up to 6 loads and 5
// stores per group); the n % 4 last elements are a scalar tail of workgroup 0.  No LDS.
// (a native vector, not HIP's float4 struct, whose store is split into four 4-byte stores and not merged again; aligned(4): a hist slot
//  starts n floats behind the previous one, and gfx950's global_load / global_store_dwordx4 take any 4-byte-aligned address)
typedef float unipc_f4 __attribute__((ext_vector_type(4), aligned(4)));
struct UniPCVec { float v[4]; };
__device__ __forceinline__ UniPCVec unipc_load(const float* p) {
    const unipc_f4 t = *reinterpret_cast<const unipc_f4*>(p);
    return UniPCVec{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void unipc_store(float* p, const UniPCVec& r) {
    unipc_f4 t;
    t.x = r.v[0]; t.y = r.v[1]; t.z = r.v[2]; t.w = r.v[3];
    *reinterpret_cast<unipc_f4*>(p) = t;
}
__device__ __forceinline__ void unipc_element(const float* c, const int pred, const float e, const float x, const float last, const float h0,
                                              const float h1, const float h2, float& m_out, float& xc_out, float& xn_out) {
#pragma clang fp contract(off)
    float m;
    if (pred == 0) {
        m = __builtin_fmaf(-c[1], e, x) / c[0];
    } else if (pred == 1) {
        const float se = c[1] * e;
        m = __builtin_fmaf(c[0], x, -se);
    } else {
        m = e;
    }
    float xc = x;
    if (c[2] != 0.f) {
        xc = c[7] * m;
        if (c[3] != 0.f) xc = __builtin_fmaf(c[3], last, xc);
        if (c[4] != 0.f) xc = __builtin_fmaf(c[4], h0, xc);
        if (c[5] != 0.f) xc = __builtin_fmaf(c[5], h1, xc);
        if (c[6] != 0.f) xc = __builtin_fmaf(c[6], h2, xc);
    }
    float xn = c[9] * m;
    if (c[8] != 0.f) xn = __builtin_fmaf(c[8], xc, xn);
    if (c[10] != 0.f) xn = __builtin_fmaf(c[10], h0, xn);
    if (c[11] != 0.f) xn = __builtin_fmaf(c[11], h1, xn);
    m_out = m; xc_out = xc; xn_out = xn;
}
__global__ void __launch_bounds__(256) sched_unipc_kernel(const UniPCParams p) {
    float c[12];
    if (p.coef_table) {
        const float* row = p.coef_table + 12 * (long long)*p.step_ptr;
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = row[j];
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) c[j] = p.coef[j];
    }
    const bool corr = c[2] != 0.f;
    const bool rd_last = corr && c[3] != 0.f, rd_h2 = corr && c[6] != 0.f;
    float* const h0p = p.hist;
    float* const h1p = p.hist + p.n;
    float* const h2p = p.hist + 2 * p.n;
    const long long groups = p.n / 4;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < groups; q += (long long)gridDim.x * 256) {
        const long long i = q * 4;
        const UniPCVec e = unipc_load(p.out + i), x = unipc_load(p.x + i);
        const UniPCVec h0 = unipc_load(h0p + i), h1 = unipc_load(h1p + i);
        UniPCVec last = {}, h2 = {}, m, xc, xn;
        if (rd_last) last = unipc_load(p.last + i);
        if (rd_h2) h2 = unipc_load(h2p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) unipc_element(c, p.pred, e.v[j], x.v[j], last.v[j], h0.v[j], h1.v[j], h2.v[j], m.v[j], xc.v[j], xn.v[j]);
        unipc_store(p.x_prev + i, xn);
        unipc_store(p.last + i, xc);
        unipc_store(h2p + i, h1);
        unipc_store(h1p + i, h0);
        unipc_store(h0p + i, m);
    }
    const long long i = groups * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < p.n) {
        const float h0 = h0p[i], h1 = h1p[i];
        float m, xc, xn;
        unipc_element(c, p.pred, p.out[i], p.x[i], rd_last ? p.last[i] : 0.f, h0, h1, rd_h2 ? h2p[i] : 0.f, m, xc, xn);
        p.x_prev[i] = xn;
        p.last[i] = xc;
        h2p[i] = h1;
        h1p[i] = h0;
        h0p[i] = m;
    }
}
int launch_sched_unipc_step(const UniPCParams& p, hipStream_t stream) {
    RLDM_REQUIRE(p.n >= 1 && p.out && p.x && p.last && p.hist && p.x_prev, "UniPC step: null argument or empty tensor");
    const long long blocks = (p.n / 4 + 255) / 256;
    const unsigned grid = (unsigned)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(sched_unipc_kernel, dim3(grid), dim3(256), 0, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

struct AddNoiseCoef { float sa[64]; float sb[64]; };
__global__ void __launch_bounds__(256) add_noise_kernel(const float* x0, const float* noise, AddNoiseCoef c, long long per,
                                                        long long n, float* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / per);
        out[i] = c.sa[b] * x0[i] + c.sb[b] * noise[i];
    }
}
int launch_add_noise(const float* x0, const float* noise, const float* sa, const float* sb, int B, long long per,
                     float* out, hipStream_t stream) {
    RLDM_REQUIRE(B <= 64, "add_noise: batch > 64");
    AddNoiseCoef c;
    for (int i = 0; i < B; ++i) { c.sa[i] = sa[i]; c.sb[i] = sb[i]; }
    const long long n = per * B;
    const unsigned grid = (unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
    hipLaunchKernelGGL(add_noise_kernel, dim3(grid), dim3(256), 0, stream, x0, noise, c, per, n, out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// DiagonalGaussianDistribution.sample (vae/sgm/modules/distributions/distributions.py:24-41), times `scale`
__global__ void __launch_bounds__(256) diag_gaussian_kernel(const float* mom, const float* noise, float scale, int z,
                                                            int spatial, long long n, float* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long per = (long long)z * spatial;
        const long long b = i / per, r = i - b * per;
        const float mean = mom[b * 2 * per + r];
        float logvar = mom[b * 2 * per + per + r];
        logvar = fminf(fmaxf(logvar, -30.0f), 20.0f);
        out[i] = (mean + expf(0.5f * logvar) * noise[i]) * scale;
    }
}
int launch_diag_gaussian(const float* moments, const float* noise, float scale, int B, int z, int spatial, float* out,
                         hipStream_t stream) {
    const long long n = (long long)B * z * spatial;
    const unsigned grid = (unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
    hipLaunchKernelGGL(diag_gaussian_kernel, dim3(grid), dim3(256), 0, stream, moments, noise, scale, z, spatial, n, out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void step_counter_kernel(int* p, int set_to, int inc) {
    if (threadIdx.x == 0) *p = (inc ? *p + inc : set_to);
}
// in-graph timeline (tools/graph_trace.py): one thread writes the constant-rate (100 MHz) real-time counter
__global__ void stamp_kernel(unsigned long long* slot) {
    if (threadIdx.x == 0) *slot = wall_clock64();
}
int launch_stamp(unsigned long long* slot, hipStream_t stream) {
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, stream, slot);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// Same-call failure signal of the persistent launches (trunk.hip): behind a sampler call's last copy, ONE workgroup reads the plan's
// self-check word and, if a cluster wait gave up during the call, overwrites ALL of the call's outputs with NaN (grid-stride over both
// buffers; the kernel returns at once when the word is clear, so the sweep is paid only by a failed call) -- a host that
// consumes the images without asking rldm_sampler_status never sees plausible-looking wrong pixels (ldm/pipelines.py:218-222, 463-464:
// the reference's contract is a correct tensor or an exception).
__global__ void __launch_bounds__(256) trunk_check_kernel(const int* err, float* a, long long na, float* b, long long nb) {
    if (*err == 0) return;
    const float nan = __int_as_float(0x7fc00000);
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < na; i += stride) a[i] = nan;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nb; i += stride) b[i] = nan;
}
int launch_trunk_check(const int* err, float* a, long long na, float* b, long long nb, hipStream_t stream) {
    hipLaunchKernelGGL(trunk_check_kernel, dim3(64), dim3(256), 0, stream, err, a, a ? na : 0, b, b ? nb : 0);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_step_counter(int* step_ptr, int set_to, int increment, hipStream_t stream) {
    hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(64), 0, stream, step_ptr, set_to, increment);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(256) scale_kernel(const float* src, float* dst, float scale, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = src[i] * scale;
}
int launch_scale_f32(const float* src, float* dst, float scale, long long n, hipStream_t stream) {
    const unsigned grid = (unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256);
    hipLaunchKernelGGL(scale_kernel, dim3(grid), dim3(256), 0, stream, src, dst, scale, n);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace rldm
