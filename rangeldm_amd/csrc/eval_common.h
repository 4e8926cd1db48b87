// eval_common.h -- what the evaluation files (chamfer, nn_index and knn through nn_stream.h, voxel, emd, fps, metrics, frechet,
// feature_metrics, lidar, rangenet_post) share, and nothing else.  No inference or training file includes it.
#pragma once
#include "common.h"

#include <initializer_list>
#include <utility>
#include <vector>

namespace rldm {

// 0, or RLDM_FRECHET_NONFINITE ("the input holds NaN or inf; nothing was computed") when one of the arrays (pointer, count;
// null entries are skipped) holds NaN / inf: one flag, one kernel (frechet.hip), one synchronise.
int check_finite_f64(std::initializer_list<std::pair<const double*, size_t>> arrays, hipStream_t st);

}  // namespace rldm

namespace {

// a device allocation that is returned to the stream's pool on every way out of a call
struct DevBuf {
    void* p = nullptr;
    hipStream_t st;
    explicit DevBuf(hipStream_t s) : st(s) {}
    ~DevBuf() { if (p) (void)hipFreeAsync(p, st); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    hipError_t alloc(size_t bytes) { return hipMallocAsync(&p, bytes, st); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Packed clouds: the offsets of one or two sets of clouds (a, and b unless dev_b is null) from the device into vectors the
// caller has sized, one synchronise for both, and what every caller requires of them.
inline int fetch_offsets(hipStream_t st, const int32_t* dev_a, std::vector<int32_t>& a, const int32_t* dev_b,
                         std::vector<int32_t>& b) {
    RLDM_HIP_CHECK(hipMemcpyAsync(a.data(), dev_a, a.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (dev_b) RLDM_HIP_CHECK(hipMemcpyAsync(b.data(), dev_b, b.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_REQUIRE(a[0] == 0 && (!dev_b || b[0] == 0), "offsets must start at 0");
    const auto nonempty = [](const std::vector<int32_t>& off) {
        for (size_t c = 0; c + 1 < off.size(); ++c)
            if (off[c + 1] <= off[c]) return false;
        return true;
    };
    RLDM_REQUIRE(nonempty(a) && (!dev_b || nonempty(b)), "every cloud must be non-empty");
    return 0;
}
inline int fetch_offsets(hipStream_t st, const int32_t* dev_a, std::vector<int32_t>& a) {
    return fetch_offsets(st, dev_a, a, nullptr, a);
}

// the segment of an ascending table that holds v: start[s] <= v < start[s + 1], for start[0] <= v < start[n]
__device__ inline int segment_of(const int* __restrict__ start, int n, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// fixed-order block sum (shuffle tree inside each wave, then the wave partials in wave order): bit-identical run to run.
// sh holds one double per wave of the workgroup.
__device__ inline double block_sum(double v, double* sh) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
    return t;
}

// One IEEE fp32 operation each, correctly rounded: plain operators under -ffp-contract=off, and sqrtf / `/` under hipcc's
// default -fhip-fp32-correctly-rounded-divide-sqrt.  (HIP's __fsqrt_rn / __fdiv_rn intrinsics are the ~1 ulp native
// instructions: measured 12 % of ranges off by one ulp against numpy.)  A file that uses them must carry
// `#pragma clang fp contract(off)` and be built with -ffp-contract=off (the Makefile's list): the pragma covers the file's own
// expressions, the flag the header inlines, which the backend would otherwise still fuse.
__device__ inline float f_mul(float a, float b) { return a * b; }
__device__ inline float f_add(float a, float b) { return a + b; }
__device__ inline float f_sub(float a, float b) { return a - b; }
__device__ inline float f_div(float a, float b) { return a / b; }
__device__ inline float f_sqrt(float a) { return sqrtf(a); }

}  // namespace
