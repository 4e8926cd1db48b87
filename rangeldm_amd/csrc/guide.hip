// guide.hip -- the measurement-consistency step of decoder-guided DDIM sampling (rangeldm_amd/guidance.py; include/rangeldm_hip.h,
// rldm_guide_*): the masked, channel-weighted squared residual of the tape decoder's reconstruction with its gradient, the update of the
// clean-latent estimate along the decoder's input gradient, and the correction of the plain DDIM step.  Element-wise fp32 with every
// rounding stated (the file is compiled with -ffp-contract=off: no product fuses with the sum it feeds) and one fp64 sum per image in
// a fixed order at every call: partial rows and a fold, never a floating-point atomic.  guidance.py restates each kernel in numpy
// (residual_host, latent_host, update_host, correct_host).
#include "train_common.h"

namespace {

using namespace rldm::train;

// element i of the NHWC tensor [B][W][H][C] -> its index in the NCHW tensor (B, C, W, H)
__device__ inline size_t guide_nchw(size_t i, int C, int W, int H) {
    const int c = (int)(i % C);
    size_t t = i / C;
    const int h = (int)(t % H);
    t /= H;
    const int w = (int)(t % W);
    const size_t b = t / W;
    return ((b * C + c) * W + w) * H + h;
}

// grid (ceil(n / 256), B), n = W H C elements per image: element 256 i + t of image b (NHWC order) is lane t of partial i of that image.
// d = xhat - y (fp32); known (m > 0.5): g = (2 wc[c]) d, one product (2 wc[c] is exact), and wc[c] d d in fp64 for the sum; unknown:
// g = +0 and +0 for the sum.  part[b][i] = block_sum_d's tree over the 256 lanes.
__global__ __launch_bounds__(256) void guide_residual_kernel(const float* __restrict__ xhat, const float* __restrict__ y,
                                                             const float* __restrict__ m, const float* __restrict__ wc, int C, int W, int H,
                                                             float* __restrict__ gx, double* __restrict__ part) {
    __shared__ double sh[4];
    const size_t n = (size_t)W * H * C;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t b = blockIdx.y;
    double v = 0.0;
    if (e < n) {
        const int c = (int)(e % C);
        const size_t px = e / C;                              // w * H + h
        const size_t i = b * n + e;
        float g = 0.f;
        if (m[b * (size_t)W * H + px] > 0.5f) {
            const float w1 = wc[c], d = xhat[i] - y[(b * C + c) * (size_t)W * H + px];
            g = (2.f * w1) * d;
            v = (double)w1 * (double)d * (double)d;
        }
        gx[i] = g;
    }
    v = block_sum_d(v, sh);
    if (threadIdx.x == 0) part[b * gridDim.x + blockIdx.x] = v;
}

// grid B: L[b] = the nparts partials of image b: thread t of 256 adds partials t, t + 256, ... in that order from +0, then block_sum_d
__global__ __launch_bounds__(256) void guide_fold_kernel(const double* __restrict__ part, int nparts, double* __restrict__ L) {
    __shared__ double sh[4];
    const double* p = part + (size_t)blockIdx.x * nparts;
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) a += p[i];
    a = block_sum_d(a, sh);
    if (threadIdx.x == 0) L[blockIdx.x] = a;
}

// the decoder's input: zin [B][W][H][C] = z0 (B, C, W, H) * inv_sf, one product
__global__ __launch_bounds__(256) void guide_latent_kernel(const float* __restrict__ z0, float inv_sf, int B, int C, int W, int H,
                                                           float* __restrict__ zin) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * W * H * C) return;
    zin[i] = z0[guide_nchw(i, C, W, H)] * inv_sf;
}

// rho_b = (float)(scale / max(sqrt(L[b]), 1e-8)) in fp64 (L null: rho = 1); t = g * inv_sf; u = rho * t; z0 = z0 - u; delta = delta + u:
// four fp32 roundings per element.  g [B][W][H][C] (the tape's gradient), z0 / delta (B, C, W, H).
__global__ __launch_bounds__(256) void guide_update_kernel(const float* __restrict__ g, const double* __restrict__ L, double scale,
                                                           float inv_sf, int B, int C, int W, int H, float* __restrict__ z0,
                                                           float* __restrict__ delta) {
    const size_t n = (size_t)W * H * C;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * n) return;
    float rho = 1.f;
    if (L) rho = (float)(scale / fmax(sqrt(L[i / n]), 1e-8));
    const float t = g[i] * inv_sf;
    const float u = rho * t;
    const size_t j = guide_nchw(i, C, W, H);
    z0[j] = z0[j] - u;
    delta[j] = delta[j] + u;
}

// p = c * delta; out = z_plain - p, and z_plain itself where p is a zero of either sign (-0 - (-0) would be +0: the bits of z_plain stay)
__global__ __launch_bounds__(256) void guide_correct_kernel(const float* __restrict__ z_plain, const float* __restrict__ delta, float c,
                                                            size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = z_plain[i], p = c * delta[i];
    out[i] = p == 0.f ? z : z - p;
}

bool guide_shape_ok(int B, int C, int W, int H) {
    return B > 0 && C > 0 && W > 0 && H > 0 && B <= 65535 && (size_t)B * C * W * H < (1ull << 40);
}

}  // namespace

extern "C" {

int rldm_guide_residual(const float* xhat, const float* y, const float* m, const float* wc, int B, int C, int W, int H, float* gx,
                        double* L, void* stream) {
    RLDM_REQUIRE(xhat && y && m && wc && gx && L, "null argument");
    RLDM_REQUIRE(guide_shape_ok(B, C, W, H), "rldm_guide_residual: B, C, W, H >= 1 and B <= 65535");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nparts = nblk((size_t)W * H * C);
    void* part = nullptr;
    if (det_partials((size_t)B * nparts * sizeof(double), st, &part)) return 1;
    guide_residual_kernel<<<dim3(nparts, (unsigned)B), 256, 0, st>>>(xhat, y, m, wc, C, W, H, gx, static_cast<double*>(part));
    TR_LAUNCH_CHECK();
    guide_fold_kernel<<<(unsigned)B, 256, 0, st>>>(static_cast<const double*>(part), (int)nparts, L);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_guide_latent(const float* z0, float inv_sf, int B, int C, int W, int H, float* zin, void* stream) {
    RLDM_REQUIRE(z0 && zin, "null argument");
    RLDM_REQUIRE(guide_shape_ok(B, C, W, H), "rldm_guide_latent: B, C, W, H >= 1");
    guide_latent_kernel<<<nblk((size_t)B * C * W * H), 256, 0, (hipStream_t)stream>>>(z0, inv_sf, B, C, W, H, zin);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_guide_update(const float* g, const double* L, double scale, float inv_sf, int B, int C, int W, int H, float* z0, float* delta,
                      void* stream) {
    RLDM_REQUIRE(g && z0 && delta, "null argument");
    RLDM_REQUIRE(guide_shape_ok(B, C, W, H), "rldm_guide_update: B, C, W, H >= 1");
    guide_update_kernel<<<nblk((size_t)B * C * W * H), 256, 0, (hipStream_t)stream>>>(g, L, scale, inv_sf, B, C, W, H, z0, delta);
    TR_LAUNCH_CHECK();
    return 0;
}

int rldm_guide_correct(const float* z_plain, const float* delta, float c, int64_t n, float* out, void* stream) {
    RLDM_REQUIRE(z_plain && delta && out && n >= 0, "null argument");
    if (n) guide_correct_kernel<<<nblk((size_t)n), 256, 0, (hipStream_t)stream>>>(z_plain, delta, c, (size_t)n, out);
    TR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
