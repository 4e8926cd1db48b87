// rangenet_post.hip -- what stands around the RangeNet++ forward, on gfx950: a scan's spherical projection into the network's
// input (LaserScan.do_range_projection + the parser's normalisation, modules/kittiparser.py:111-171, 391-395) and the way
// back from the per-pixel argmax to per-point labels (User.infer_subset's `proj_argmax[p_y, p_x]`, or postproc/KNN.py).
//
//   scan_keys_kernel      one thread per point: depth, pixel, and the point's bid for its pixel (64-bit atomicMin)
//   scan_finish_kernel    one thread per pixel: the winner's range / xyz / remission, normalised and masked
//   unproject_kernel<S,K> one thread per point: the label of its pixel, or the KNN vote over an S x S window
//
// All of it is memory bound fp32.  Every arithmetic step is one correctly rounded fp32 operation in the reference's order
// (no FMA contraction: the pragma below and the Makefile), so that numpy restates it exactly: rangenet.scatter_host and
// rangenet.knn_labels_host.  The two libm calls (atan2f, asinf) are the exception: a pixel may differ from numpy's where the
// coordinate lies within a few ulp of an integer.
//
// Clouds come as a ragged batch: points [sum N][stride] fp32 (x, y, z, remission if stride >= 4) and offsets [B + 1] on the
// device.  No entry point reads the offsets on the host: the grids are fixed (blockIdx.y is the cloud, the threads of a row
// stride over its points), nothing is allocated and nothing synchronises.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) what eval_common.h's f_* operators need

namespace {

typedef unsigned long long u64;

constexpr int SCAN_BLOCKS_X = 128;          // blocks of 256 threads that stride over one cloud's points

struct ScanDev {
    int H, W, stride;
    float fov_down_abs, fov;                // |fov_down| and |fov_down| + |fov_up| in radians, rounded from fp64
    float pi;                               // (float)M_PI: what numpy makes of np.pi beside a float32 array
    float mean[5], std[5];
};

// kittiparser.py:123-151 (rangenet.project_scan lines 317-326), expression by expression
__global__ __launch_bounds__(256) void scan_keys_kernel(const float* __restrict__ pts, const int* __restrict__ off, ScanDev S,
                                                        u64* __restrict__ keys, int* __restrict__ px_out,
                                                        int* __restrict__ py_out, float* __restrict__ range_out) {
    const int b = blockIdx.y;
    const int q0 = off[b], n = off[b + 1] - q0;
    u64* __restrict__ k = keys + (size_t)b * S.H * S.W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += SCAN_BLOCKS_X * 256) {
        const float* p = pts + (size_t)(q0 + i) * S.stride;
        const float x = p[0], y = p[1], z = p[2];
        const float depth = f_sqrt(f_add(f_add(f_mul(x, x), f_mul(y, y)), f_mul(z, z)));
        int px = -1, py = -1;
        if (depth > 0.f && depth < INFINITY) {          // a zero or non-finite return never competes (NaN fails both)
            const float yaw = -atan2f(y, x);
            const float pitch = asinf(f_div(z, depth));
            float fx = f_mul(0.5f, f_add(f_div(yaw, S.pi), 1.0f));
            float fy = f_sub(1.0f, f_div(f_add(pitch, S.fov_down_abs), S.fov));
            fx = floorf(f_mul(fx, (float)S.W));
            fy = floorf(f_mul(fy, (float)S.H));
            fx = fmaxf(0.f, fminf((float)(S.W - 1), fx));
            fy = fmaxf(0.f, fminf((float)(S.H - 1), fy));
            px = (int)fx;
            py = (int)fy;
            // nearest wins; among equal depths the lowest index (positive floats order like their bit patterns)
            atomicMin(k + (size_t)py * S.W + px, ((u64)__float_as_uint(depth) << 32) | (unsigned)i);
        }
        if (px_out) px_out[q0 + i] = px;
        if (py_out) py_out[q0 + i] = py;
        if (range_out) range_out[q0 + i] = depth;
    }
}

// the winner of every pixel -> proj (B, 5, H, W) = ((value - mean) / std) * mask, and the raw images KNN needs
__global__ __launch_bounds__(256) void scan_finish_kernel(const u64* __restrict__ keys, const float* __restrict__ pts,
                                                          const int* __restrict__ off, ScanDev S, float* __restrict__ proj,
                                                          float* __restrict__ mask_out, float* __restrict__ range_out,
                                                          int* __restrict__ idx_out) {
    const int b = blockIdx.y;
    const int HW = S.H * S.W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const u64 key = keys[(size_t)b * HW + i];
    float v[5] = {-1.f, -1.f, -1.f, -1.f, -1.f};
    int idx = -1;
    if (key != ~0ull) {
        idx = (int)(unsigned)key;
        const float* p = pts + (size_t)(off[b] + idx) * S.stride;
        v[0] = __uint_as_float((unsigned)(key >> 32));
        v[1] = p[0]; v[2] = p[1]; v[3] = p[2];
        v[4] = S.stride >= 4 ? p[3] : 0.f;
    }
    const float m = idx > 0 ? 1.f : 0.f;                // the reference's `proj_idx > 0`: point 0's pixel is dropped too
    float* o = proj + (size_t)b * 5 * HW + i;
#pragma unroll
    for (int c = 0; c < 5; ++c) o[(size_t)c * HW] = f_mul(f_div(f_sub(v[c], S.mean[c]), S.std[c]), m);
    if (mask_out) mask_out[(size_t)b * HW + i] = m;
    if (range_out) range_out[(size_t)b * HW + i] = v[0];
    if (idx_out) idx_out[(size_t)b * HW + i] = idx;
}

// ---- labels back to the points ------------------------------------------------------------------------------------------
// postproc/KNN.py forward for one point.  The S x S window entries are visited in the order of F.unfold's rows,
// k = dy * S + dx; the K nearest are kept sorted in registers by an insertion that moves an entry only past strictly larger
// ones, so equal distances stay in window order.  Slot j >= (entries seen so far) is empty and takes anything: an infinite
// distance is kept like any other.  K is the number of slots (>= knn); every loop is unrolled, nothing is indexed dynamically.
struct KnnDev {
    int H, W, knn, num_classes;
    float cutoff;
};

template <int S, int K>
__device__ __forceinline__ int knn_vote(const float* __restrict__ rng, const unsigned char* __restrict__ lab, int px, int py,
                                        float r, const float* __restrict__ wgt, const KnnDev& P) {
    float d[K];
    int l[K];
    constexpr int R = S / 2;
#pragma unroll
    for (int k = 0; k < S * S; ++k) {
        const int yy = py + k / S - R, xx = px + k % S - R;
        float e = 0.f;                                  // F.unfold pads with zeros: range 0 and label 0 outside the image
        int c = 0;
        if (yy >= 0 && yy < P.H && xx >= 0 && xx < P.W) {
            e = rng[(size_t)yy * P.W + xx];
            c = lab[(size_t)yy * P.W + xx];
            if (e < 0.f) e = INFINITY;
        }
        if (k == (S * S - 1) / 2) e = r;                // the centre is the point itself
        const float dist = f_mul(fabsf(f_sub(e, r)), wgt[k]);
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            if (j > k) continue;                        // (compile time) slots past the entries seen stay empty
            const bool here = j >= k || dist < d[j];    // the entry belongs at slot j or before it
            const bool before = j > 0 && (j - 1 >= k || dist < d[j - 1]);
            if (j >= k) {                               // (compile time) the first empty slot
                d[j] = before ? d[j > 0 ? j - 1 : 0] : dist;
                l[j] = before ? l[j > 0 ? j - 1 : 0] : c;
            } else {
                d[j] = here ? (before ? d[j > 0 ? j - 1 : 0] : dist) : d[j];
                l[j] = here ? (before ? l[j > 0 ? j - 1 : 0] : c) : l[j];
            }
        }
    }
    // votes: 8 bits per class, eight classes per word (knn <= 49 < 256, num_classes <= 32)
    u64 cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool counts = j < P.knn && l[j] > 0 && l[j] < P.num_classes && !(P.cutoff > 0.f && d[j] > P.cutoff);
        const u64 one = counts ? 1ull << ((l[j] & 7) * 8) : 0ull;
#pragma unroll
        for (int w = 0; w < 4; ++w) cnt[w] += (l[j] >> 3) == w ? one : 0ull;
    }
    int best = 1, best_n = -1;
#pragma unroll
    for (int c = 1; c < 32; ++c) {
        const int n = (int)((cnt[c >> 3] >> ((c & 7) * 8)) & 255);
        if (c < P.num_classes && n > best_n) { best_n = n; best = c; }      // a strict >: the lowest class on ties
    }
    return best;
}

template <int S, int K>
__global__ __launch_bounds__(256) void unproject_kernel(const float* __restrict__ proj_range, const unsigned char* __restrict__ argmax,
                                                        const int* __restrict__ px, const int* __restrict__ py,
                                                        const float* __restrict__ unproj_range, const int* __restrict__ off,
                                                        const float* __restrict__ wgt, KnnDev P, unsigned char* __restrict__ labels) {
    const int b = blockIdx.y;
    const int q0 = off[b], n = off[b + 1] - q0;
    const size_t img = (size_t)b * P.H * P.W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += SCAN_BLOCKS_X * 256) {
        const int x = px[q0 + i], y = py[q0 + i];
        int out = 0;
        if (x >= 0 && x < P.W && y >= 0 && y < P.H) {   // (a dropped point carries -1)
            if constexpr (S == 0) out = argmax[img + (size_t)y * P.W + x];
            else out = knn_vote<S, K>(proj_range + img, argmax + img, x, y, unproj_range[q0 + i], wgt, P);
        }
        labels[q0 + i] = (unsigned char)out;
    }
}

}  // namespace

extern "C" {

int rldm_rangenet_project(const float* points, const int32_t* offsets, int B, int stride, int H, int W, double fov_up,
                          double fov_down, const float* means, const float* stds, uint64_t* keys_workspace, float* proj,
                          float* mask, float* proj_range, int32_t* proj_idx, int32_t* px, int32_t* py, float* unproj_range,
                          void* stream) {
    RLDM_REQUIRE(points && offsets && means && stds && keys_workspace && proj, "null argument");
    RLDM_REQUIRE(B > 0 && B <= 65535 && stride >= 3 && H > 0 && W > 0, "bad shape");
    RLDM_REQUIRE((long long)B * 5 * H * W < (1LL << 31), "the projected batch must stay below 2^31 elements");
    ScanDev S;
    S.H = H; S.W = W; S.stride = stride;
    const double up = fov_up / 180.0 * M_PI, down = fov_down / 180.0 * M_PI;     // kittiparser.py:118-120, python floats
    S.fov_down_abs = (float)std::fabs(down);
    S.fov = (float)(std::fabs(down) + std::fabs(up));
    S.pi = (float)M_PI;
    RLDM_REQUIRE(S.fov > 0.f, "the field of view is empty");
    for (int c = 0; c < 5; ++c) { S.mean[c] = means[c]; S.std[c] = stds[c]; }
    hipStream_t st = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    RLDM_HIP_CHECK(hipMemsetAsync(keys_workspace, 0xff, (size_t)B * HW * sizeof(u64), st));
    scan_keys_kernel<<<dim3(SCAN_BLOCKS_X, B), 256, 0, st>>>(points, offsets, S, reinterpret_cast<u64*>(keys_workspace), px, py,
                                                            unproj_range);
    RLDM_HIP_CHECK(hipGetLastError());
    scan_finish_kernel<<<dim3((unsigned)((HW + 255) / 256), B), 256, 0, st>>>(reinterpret_cast<const u64*>(keys_workspace), points,
                                                                              offsets, S, proj, mask, proj_range, proj_idx);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_rangenet_unproject(const float* proj_range, const uint8_t* argmax, const int32_t* px, const int32_t* py,
                            const float* unproj_range, const int32_t* offsets, int B, int H, int W, int knn, int search,
                            const float* weights, float cutoff, int num_classes, uint8_t* labels, void* stream) {
    RLDM_REQUIRE(argmax && px && py && offsets && labels, "null argument");
    RLDM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "bad shape");
    RLDM_REQUIRE((long long)B * H * W < (1LL << 31), "the batch of images must stay below 2^31 pixels");
    RLDM_REQUIRE(knn >= 0, "knn must not be negative");
    KnnDev P;
    P.H = H; P.W = W; P.knn = knn; P.num_classes = num_classes; P.cutoff = cutoff;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(SCAN_BLOCKS_X, B);
#define RLDM_UNPROJECT(S, K)                                                                                              \
    unproject_kernel<S, K><<<grid, 256, 0, st>>>(proj_range, argmax, px, py, unproj_range, offsets, weights, P, labels)
    if (knn == 0) {
        RLDM_UNPROJECT(0, 0);
    } else {
        RLDM_REQUIRE(proj_range && unproj_range && weights, "KNN needs proj_range, unproj_range and the window weights");
        RLDM_REQUIRE(search == 1 || search == 3 || search == 5 || search == 7, "search must be odd and at most 7");
        RLDM_REQUIRE(knn <= search * search, "knn exceeds the search window");
        RLDM_REQUIRE(num_classes >= 2 && num_classes <= 32, "num_classes must be in [2, 32]");
        RLDM_REQUIRE(cutoff >= 0.f, "cutoff must not be negative (0: none)");
        if (search == 1) RLDM_UNPROJECT(1, 1);
        else if (search == 3) RLDM_UNPROJECT(3, 9);
        else if (search == 5 && knn <= 8) RLDM_UNPROJECT(5, 8);
        else if (search == 5) RLDM_UNPROJECT(5, 25);
        else if (knn <= 8) RLDM_UNPROJECT(7, 8);
        else RLDM_UNPROJECT(7, 49);
    }
#undef RLDM_UNPROJECT
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
