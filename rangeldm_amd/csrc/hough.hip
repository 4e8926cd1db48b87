// hough.hip -- a sensor's per-beam tables (mounting height, inclination) from its own sweeps on gfx950: the Hough vote the
// RangeLDM paper derives its hole-free range images with, and the assignment and moments behind the per-beam line fit.
//
//   hough_pack_kernel      (x, y, z) -> (d, z), d = sqrt(x^2 + y^2); d = -1 marks a point that takes no part
//   hough_vote_kernel      every valid point votes once per inclination row: the hot path
//   hough_row_max_kernel   per row the largest count and the lowest h bin holding it
//   hough_assign_kernel    per point the candidate beam with the smallest residual in tangent space
//   hough_moments_kernel   per beam and slice of points: n, sum d, sum z, sum d^2, sum d z in fp64
//   hough_moments_sum      the slice partials added in slice order
//
// Model.  A return of beam k satisfies atan2(height_k - z, d) = incl_k (ldm/kitti360_range_image.py:51-61, to_pc_torch), so
// with t = tan(incl):  h = z + d t.  A return is a line in the (t, h) plane with slope d; the returns of one beam meet at
// (tan(incl_k), height_k).  Range noise moves a return along its ray, that is along its line.
//
// Arithmetic.  Every fp32 expression is one correctly rounded operation (eval_common.h's f_mul .. f_sqrt; the Makefile gives
// this file -ffp-contract=off, -fhip-fp32-correctly-rounded-divide-sqrt and -fno-gpu-flush-denormals-to-zero), and there is no
// transcendental on the device: the tangents of the rows and of the candidate beams come from the host as a table.  numpy
// restates pack, vote, row_max and assign bit for bit (rangeldm_amd/sensor.py: hough_votes_host, row_peaks_host, assign_host).
//
// Vote.  A workgroup of 256 threads owns ROWS consecutive inclination rows and one slice of the packed points.  It keeps the
// rows' histograms in LDS (ROWS x n_h counters, HOUGH_LDS_CELLS = 8 192 at most: a static 32 KiB, so five workgroups, 20
// waves, share a CU's 160 KiB), reads each point once (one 8-byte load per lane, coalesced), computes the ROWS bins with the row tangents in scalar registers, and votes with LDS integer atomics.
// A vote is cast only after its bin index passed 0 <= jf < n_h as a float, so NaN, inf and 1e30 never reach the cast or an
// address.  At the end the workgroup adds its non-zero counters into acc with global integer atomics.  Integers: the result
// does not depend on the order of anything.  ROWS = min(8, 8192 / n_h): eight rows keep the per-point work (one load, eight
// multiply-add-scale-floor chains) in registers, and leave 300 row blocks for the default 2 400-row grid, which with slices of
// at least HOUGH_MIN_SLICE = 1 024 points fills the chip from one sweep upwards.  Peak rows: in the row of a beam's own
// inclination every return of that beam lands in one counter; the lanes of a wave hold different beams' returns there (a
// sweep interleaves beams), so a counter sees a few lanes of a wave, and the LDS serialises only those.  The worst case,
// all 64 lanes on one counter (identical points), costs 64 LDS cycles per vote and is still exact.
//
// Moments.  fp64, no floating-point atomics, a fixed order: a workgroup owns HOUGH_MOM_BEAMS = 4 beams and one slice of the
// points; lanes stride over the slice and accumulate in registers (values are converted to fp64 before any product), the lane
// partials are summed by eval_common.h's fixed-order block_sum, and hough_moments_sum adds the slice partials in slice order.
// The slicing depends on n alone, so two calls give the same bits.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) z + d * t is two IEEE operations, never an fma

namespace {

constexpr int HOUGH_THREADS = 256;
constexpr int HOUGH_LDS_CELLS = 8192;                        // counters of one workgroup's rows: 32 KiB
constexpr int HOUGH_MAX_ROWS = 8;                            // rows of one workgroup
constexpr long long HOUGH_MIN_SLICE = 1024;                  // points of one slice, at least (a multiple of HOUGH_THREADS)
constexpr long long HOUGH_TARGET_WGS = 4096;                 // workgroups a large call is cut into (16 per CU)
constexpr int HOUGH_MAX_SLICES = 65535;                      // gridDim.y
constexpr int HOUGH_MOM_BEAMS = 4;                           // beams of one moments workgroup
constexpr long long HOUGH_MOM_SLICE = 8192;                  // points of one moments slice, at least
constexpr int HOUGH_MOM_MAX_SLICES = 1024;

int vote_rows(int n_h) { return std::max(1, std::min(HOUGH_MAX_ROWS, HOUGH_LDS_CELLS / n_h)); }

long long vote_slice(long long n, int n_t, int n_h) {
    const int rows = vote_rows(n_h);
    const long long row_blocks = (n_t + rows - 1) / rows;
    long long slices = std::max<long long>(1, std::min<long long>(HOUGH_MAX_SLICES, HOUGH_TARGET_WGS / row_blocks));
    long long len = std::max(HOUGH_MIN_SLICE, (n + slices - 1) / slices);
    len = (len + HOUGH_THREADS - 1) / HOUGH_THREADS * HOUGH_THREADS;
    while ((n + len - 1) / len > HOUGH_MAX_SLICES) len *= 2;
    return len;
}

__global__ __launch_bounds__(HOUGH_THREADS) void hough_pack_kernel(const float* __restrict__ pts, long long n, int stride,
                                                                   float d_min, float d_max, float2* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * HOUGH_THREADS + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    const float d = f_sqrt(f_add(f_mul(x, x), f_mul(y, y)));
    // finite x, y, z (NaN fails every comparison), and d inside [d_min, d_max], both ends included
    const bool ok = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY && d >= d_min && d <= d_max;
    packed[i] = make_float2(ok ? d : -1.0f, z);
}

// grid (row blocks, slices).  Block (bx, by) owns rows [bx * rows, min(n_t, (bx + 1) * rows)) and points
// [by * slice, min(n, (by + 1) * slice)).  rows * n_h <= HOUGH_LDS_CELLS (the host checks it).
__global__ __launch_bounds__(HOUGH_THREADS) void hough_vote_kernel(const float2* __restrict__ packed, long long n,
                                                                   long long slice, const float* __restrict__ tan_table,
                                                                   int n_t, int rows, float h_min, float inv_dh, int n_h,
                                                                   unsigned* __restrict__ acc) {
    __shared__ unsigned hist[HOUGH_LDS_CELLS];
    const int row0 = blockIdx.x * rows;
    const int mine = min(rows, n_t - row0);                  // >= 1: the grid has ceil(n_t / rows) row blocks
    const int cells = mine * n_h;
    for (int c = threadIdx.x; c < cells; c += HOUGH_THREADS) hist[c] = 0u;
    float t[HOUGH_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < HOUGH_MAX_ROWS; ++r) t[r] = tan_table[row0 + min(r, mine - 1)];      // uniform: scalar registers
    __syncthreads();
    const long long p0 = (long long)blockIdx.y * slice, p1 = min(n, p0 + slice);
    const float fn_h = (float)n_h;                           // n_h <= 4096: exact
    for (long long i = p0 + threadIdx.x; i < p1; i += HOUGH_THREADS) {
        const float2 p = packed[i];
        if (!(p.x >= 0.0f)) continue;                        // d = -1: the point takes no part
#pragma unroll
        for (int r = 0; r < HOUGH_MAX_ROWS; ++r) {
            if (r < mine) {
                const float h = f_add(p.y, f_mul(p.x, t[r]));
                const float jf = floorf(f_mul(f_sub(h, h_min), inv_dh));
                if (jf >= 0.0f && jf < fn_h) atomicAdd(&hist[r * n_h + (int)jf], 1u);        // compared as floats first
            }
        }
    }
    __syncthreads();
    unsigned* out = acc + (size_t)row0 * n_h;
    for (int c = threadIdx.x; c < cells; c += HOUGH_THREADS) {
        const unsigned v = hist[c];
        if (v) atomicAdd(out + c, v);
    }
}

// one workgroup per row: (count, bin) with the larger count, on equal counts the lower bin
__global__ __launch_bounds__(HOUGH_THREADS) void hough_row_max_kernel(const unsigned* __restrict__ acc, int n_h,
                                                                      unsigned* __restrict__ row_max, int* __restrict__ row_arg) {
    __shared__ unsigned sv[HOUGH_THREADS];
    __shared__ int sj[HOUGH_THREADS];
    const unsigned* row = acc + (size_t)blockIdx.x * n_h;
    unsigned best = 0u;
    int arg = 0;
    for (int j = threadIdx.x; j < n_h; j += HOUGH_THREADS) {                 // ascending j: `>` keeps the lowest bin
        const unsigned v = row[j];
        if (v > best) { best = v; arg = j; }
    }
    sv[threadIdx.x] = best;
    sj[threadIdx.x] = arg;
    __syncthreads();
    for (int o = HOUGH_THREADS / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const unsigned v = sv[threadIdx.x + o];
            const int j = sj[threadIdx.x + o];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && v != 0u && j < sj[threadIdx.x])) {
                sv[threadIdx.x] = v;
                sj[threadIdx.x] = j;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        row_max[blockIdx.x] = sv[0];
        row_arg[blockIdx.x] = sv[0] ? sj[0] : 0;
    }
}

// cand: [beams][2] = (tan_k, h_k), beams <= 256
__global__ __launch_bounds__(HOUGH_THREADS) void hough_assign_kernel(const float2* __restrict__ packed, long long n,
                                                                     const float2* __restrict__ cand, int beams, float tol,
                                                                     short* __restrict__ ids) {
    __shared__ float2 sc[256];
    if ((int)threadIdx.x < beams) sc[threadIdx.x] = cand[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * HOUGH_THREADS + threadIdx.x;
    if (i >= n) return;
    const float2 p = packed[i];
    float best = INFINITY;
    int id = -1;
    if (p.x >= 0.0f) {
        for (int k = 0; k < beams; ++k) {
            const float e = fabsf(f_sub(f_div(f_sub(sc[k].y, p.y), p.x), sc[k].x));
            if (e < best) { best = e; id = k; }              // strict: the lowest k keeps a tie; NaN is never taken
        }
    }
    ids[i] = (short)(best < tol ? id : -1);
}

// grid (beam groups, slices); part: [slices][beams][5] = n, sum d, sum z, sum d^2, sum d z (n as an exact fp64 integer)
__global__ __launch_bounds__(HOUGH_THREADS) void hough_moments_kernel(const float2* __restrict__ packed,
                                                                      const short* __restrict__ ids, long long n,
                                                                      long long slice, int beams, double* __restrict__ part) {
    __shared__ double sh[HOUGH_THREADS / 64];
    const int b0 = blockIdx.x * HOUGH_MOM_BEAMS;
    double a[HOUGH_MOM_BEAMS][5];
#pragma unroll
    for (int b = 0; b < HOUGH_MOM_BEAMS; ++b)
#pragma unroll
        for (int q = 0; q < 5; ++q) a[b][q] = 0.0;
    const long long p0 = (long long)blockIdx.y * slice, p1 = min(n, p0 + slice);
    for (long long i = p0 + threadIdx.x; i < p1; i += HOUGH_THREADS) {
        const int k = (int)ids[i] - b0;
        if (k < 0 || k >= HOUGH_MOM_BEAMS) continue;
        const float2 p = packed[i];
        const double d = (double)p.x, z = (double)p.y;
        const double dd = d * d, dz = d * z;
#pragma unroll
        for (int b = 0; b < HOUGH_MOM_BEAMS; ++b) {
            if (b == k) {
                a[b][0] += 1.0; a[b][1] += d; a[b][2] += z; a[b][3] += dd; a[b][4] += dz;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < HOUGH_MOM_BEAMS; ++b) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double s = block_sum(a[b][q], sh);
            if (threadIdx.x == 0 && b0 + b < beams) part[((size_t)blockIdx.y * beams + (b0 + b)) * 5 + q] = s;
        }
    }
}

// one thread per (beam, moment): the slices in slice order
__global__ __launch_bounds__(HOUGH_THREADS) void hough_moments_sum(const double* __restrict__ part, int slices, int beams,
                                                                   long long* __restrict__ counts, double* __restrict__ sums) {
    const int e = blockIdx.x * HOUGH_THREADS + threadIdx.x;
    if (e >= beams * 5) return;
    double s = 0.0;
    for (int y = 0; y < slices; ++y) s += part[(size_t)y * beams * 5 + e];
    const int b = e / 5, q = e % 5;
    if (q == 0) counts[b] = (long long)s;                    // a sum of ones below 2^53: exact
    else sums[b * 4 + (q - 1)] = s;
}

}  // namespace

extern "C" {

int rldm_hough_pack(const float* points, int64_t n, int stride, float d_min, float d_max, float* packed, void* stream) {
    RLDM_REQUIRE(n >= 0 && n < (1LL << 31) && stride >= 3, "bad shape");
    RLDM_REQUIRE(d_min >= 0.0f && d_max >= d_min && std::isfinite(d_max), "0 <= d_min <= d_max < inf");
    if (n == 0) return 0;
    RLDM_REQUIRE(points && packed, "null argument");
    hough_pack_kernel<<<(unsigned)((n + HOUGH_THREADS - 1) / HOUGH_THREADS), HOUGH_THREADS, 0, (hipStream_t)stream>>>(
        points, n, stride, d_min, d_max, reinterpret_cast<float2*>(packed));
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_hough_vote_shape(int64_t n, int n_theta, int n_h, int32_t* rows, int64_t* slice) {
    RLDM_REQUIRE(n >= 0 && n < (1LL << 31) && n_theta >= 1 && n_theta <= RLDM_HOUGH_MAX_THETA && n_h >= 1 && n_h <= RLDM_HOUGH_MAX_H,
                 "bad shape");
    RLDM_REQUIRE(rows && slice, "null argument");
    *rows = vote_rows(n_h);
    *slice = vote_slice(n, n_theta, n_h);
    return 0;
}

int rldm_hough_vote(const float* packed, int64_t n, const float* tan_table, int n_theta, float h_min, float inv_dh, int n_h,
                    uint32_t* acc, void* stream) {
    RLDM_REQUIRE(n >= 0 && n < (1LL << 31) && n_theta >= 1 && n_theta <= RLDM_HOUGH_MAX_THETA && n_h >= 1 && n_h <= RLDM_HOUGH_MAX_H,
                 "bad shape");
    RLDM_REQUIRE(std::isfinite(h_min) && inv_dh > 0.0f && std::isfinite(inv_dh), "h_min finite, inv_dh positive and finite");
    if (n == 0) return 0;
    RLDM_REQUIRE(packed && tan_table && acc, "null argument");
    const int rows = vote_rows(n_h);
    RLDM_REQUIRE(rows >= 1 && rows <= HOUGH_MAX_ROWS && (long long)rows * n_h <= HOUGH_LDS_CELLS, "internal: rows of a workgroup");
    const long long slice = vote_slice(n, n_theta, n_h);
    const dim3 grid((unsigned)((n_theta + rows - 1) / rows), (unsigned)((n + slice - 1) / slice));
    RLDM_REQUIRE(grid.y >= 1 && grid.y <= (unsigned)HOUGH_MAX_SLICES, "internal: slices");
    hough_vote_kernel<<<grid, HOUGH_THREADS, 0, (hipStream_t)stream>>>(reinterpret_cast<const float2*>(packed), n, slice,
                                                                      tan_table, n_theta, rows, h_min, inv_dh, n_h, acc);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_hough_row_max(const uint32_t* acc, int n_theta, int n_h, uint32_t* row_max, int32_t* row_arg, void* stream) {
    RLDM_REQUIRE(acc && row_max && row_arg, "null argument");
    RLDM_REQUIRE(n_theta >= 1 && n_theta <= RLDM_HOUGH_MAX_THETA && n_h >= 1 && n_h <= RLDM_HOUGH_MAX_H, "bad shape");
    hough_row_max_kernel<<<n_theta, HOUGH_THREADS, 0, (hipStream_t)stream>>>(acc, n_h, row_max, row_arg);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_hough_assign(const float* packed, int64_t n, const float* candidates, int beams, float tol, int16_t* ids, void* stream) {
    RLDM_REQUIRE(n >= 0 && n < (1LL << 31) && beams >= 1 && beams <= RLDM_HOUGH_MAX_BEAMS, "bad shape");
    RLDM_REQUIRE(tol > 0.0f, "tol must be positive");
    if (n == 0) return 0;
    RLDM_REQUIRE(packed && candidates && ids, "null argument");
    hough_assign_kernel<<<(unsigned)((n + HOUGH_THREADS - 1) / HOUGH_THREADS), HOUGH_THREADS, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float2*>(packed), n, reinterpret_cast<const float2*>(candidates), beams, tol, ids);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_hough_moments(const float* packed, const int16_t* ids, int64_t n, int beams, int64_t* counts, double* sums,
                       void* stream) {
    RLDM_REQUIRE(n >= 0 && n < (1LL << 31) && beams >= 1 && beams <= RLDM_HOUGH_MAX_BEAMS, "bad shape");
    RLDM_REQUIRE(counts && sums, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        RLDM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)beams * sizeof(int64_t), st));
        RLDM_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)beams * 4 * sizeof(double), st));
        return 0;
    }
    RLDM_REQUIRE(packed && ids, "null argument");
    long long slice = std::max<long long>(HOUGH_MOM_SLICE, (n + HOUGH_MOM_MAX_SLICES - 1) / HOUGH_MOM_MAX_SLICES);
    slice = (slice + HOUGH_THREADS - 1) / HOUGH_THREADS * HOUGH_THREADS;
    const int slices = (int)((n + slice - 1) / slice);       // <= HOUGH_MOM_MAX_SLICES; a function of n alone
    DevBuf pbuf(st);
    RLDM_HIP_CHECK(pbuf.alloc((size_t)slices * beams * 5 * sizeof(double)));
    const dim3 grid((unsigned)((beams + HOUGH_MOM_BEAMS - 1) / HOUGH_MOM_BEAMS), (unsigned)slices);
    hough_moments_kernel<<<grid, HOUGH_THREADS, 0, st>>>(reinterpret_cast<const float2*>(packed), ids, n, slice, beams,
                                                        pbuf.as<double>());
    RLDM_HIP_CHECK(hipGetLastError());
    hough_moments_sum<<<(beams * 5 + HOUGH_THREADS - 1) / HOUGH_THREADS, HOUGH_THREADS, 0, st>>>(
        pbuf.as<double>(), slices, beams, reinterpret_cast<long long*>(counts), sums);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
