// chamfer.hip -- reconstruction metrics on gfx950: the Chamfer distance of ldm/convert_vae.py:262-271
// (pytorch3d.loss.chamfer_distance with its defaults: norm=2, point_reduction="mean", batch_reduction="mean") and the
// range-image errors / beam-upsampling baselines of ldm/convert_vae.py:236-247 and metrics/metrics/mae.py:45-117.
//
//   chamfer_nn_kernel      for every query point the SQUARED distance to its nearest neighbour in the other cloud of its pair
//   chamfer_mean_kernel    per pair and direction the mean of those minima, fp64, fixed order
//   chamfer_matrix_kernel  one direction of the ALL-PAIRS matrix between two sets of clouds: a workgroup keeps one query block
//                          in registers and streams a run of target clouds past it, one fp64 block sum per (i, j, block)
//   matrix_finish_kernel   those block sums added in block order and divided once -> xy / yx
//   row_argmin_kernel      per row of an fp64 matrix the minimum and the LOWEST column attaining it
//   range_errors_kernel    per image fp64 sum |a - b| and sum (a - b)^2 after a per-channel affine map, over a channel set and
//                          an azimuth window that may wrap past the seam
//   beam_upsample_kernel   (B, C, W, Hs) -> (B, C, W, Hs * rate) along the beam axis: cv2 INTER_NEAREST / INTER_CUBIC
//
// Nearest-neighbour numerics and the streaming loop are nn_stream.h's (see its header): d^2 = ((dx*dx + dy*dy) + dz*dz), every
// operation one IEEE fp32 rounding, so every per-point minimum is bit-equal to a CPU fp32 evaluation of the same expression.
//
// Structure.  A chamfer_nn_kernel workgroup owns one query block of one pair and one contiguous chunk of that pair's target
// cloud.  Long target clouds are split over several workgroups so that a handful of pairs still fills the chip; the partial
// minima are merged with atomicMin on the bit pattern (non-negative floats order like uint32), so the result does not depend
// on the split.
//
// Preconditions: clouds are non-empty (the Python layer raises ValueError); coordinates are finite -- NaN or inf inputs
// give unspecified results (not checked).
#include "nn_stream.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d^2 and the cubic weights are single IEEE ops

namespace {

// grid: one workgroup per (pair, query block, target chunk); wg_start[p] = first workgroup of pair p (num_pairs + 1 entries).
// out (pre-filled with +inf) receives atomicMin of the float bit patterns, indexed like the packed query array.  Eight waves
// per SIMD: the loop's state fits 64 VGPRs, and saying so keeps the sweep's tile reads from being hoisted into 84.
__global__ __launch_bounds__(NN_THREADS, 8) void chamfer_nn_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                                   int qstride, const float* __restrict__ t,
                                                                   const int* __restrict__ toff, int tstride, int num_pairs,
                                                                   const int* __restrict__ wg_start, int splits,
                                                                   unsigned* __restrict__ out) {
    __shared__ float4 tile[NN_TILE];
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int p = segment_of(wg_start, num_pairs, wg);
    const int q0 = qoff[p], nq = qoff[p + 1] - q0, t0 = toff[p], nt = toff[p + 1] - t0;
    const int sp = pair_splits(splits, nt);
    const int local = wg - wg_start[p];
    const int qb = local / sp, s = local - qb * sp;
    const int chunk = (nt + sp - 1) / sp;
    const int t_begin = s * chunk, t_end = min(nt, t_begin + chunk);

    const PackedQueries pq = load_queries(q, q0, nq, qstride, qb, tid);
    f2 best[NN_R / 2];
#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) best[k] = f2{INFINITY, INFINITY};
    for (int base = t_begin; base < t_end; base += NN_TILE) {
        const int n4 = stage_tile(tile, t, t0 + base, min(NN_TILE, t_end - base), tstride, tid);
        sweep_tile(tile, 0, n4, pq, best);
    }

#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = qb * NN_QB + (2 * k + h) * NN_THREADS + tid;
            if (i < nq) atomicMin(out + q0 + i, __float_as_uint(h ? best[k].y : best[k].x));
        }
    }
}

// grid (num_pairs, 2): y = 0 the x -> y direction, 1 the y -> x direction
__global__ __launch_bounds__(256) void chamfer_mean_kernel(const float* __restrict__ xd, const int* __restrict__ xoff,
                                                           const float* __restrict__ yd, const int* __restrict__ yoff,
                                                           double* __restrict__ xmean, double* __restrict__ ymean) {
    __shared__ double sh[4];
    const int p = blockIdx.x;
    const float* d = blockIdx.y ? yd : xd;
    const int* off = blockIdx.y ? yoff : xoff;
    const int b = off[p], e = off[p + 1];
    double acc = 0.0;
    for (int i = b + threadIdx.x; i < e; i += 256) acc += (double)d[i];
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) (blockIdx.y ? ymean : xmean)[p] = acc / (double)(e - b);
}

// ---- all-pairs matrix -----------------------------------------------------------------------------------------------
// One direction: query set Q (nq clouds), target set T (nt clouds).  Workgroup = (query block g, run r): the block's NN_QB
// points stay in registers while the target clouds [r * run, (r + 1) * run) -- in the symmetric case only those above
// (tri > 0) or below (tri < 0) the query cloud -- stream through the LDS tile under nn_stream.h's sweep.  A target
// cloud is never split, so each minimum is final when its cloud ends: the block then adds its minima in fp64 (per thread in
// slot order, block_sum across threads) into part[qb_start[c] * nt + j * nqb(c) + qb].  That sum depends on (c, qb, j)
// alone -- not on `run`, the grid, or which other clouds the call holds.
__global__ __launch_bounds__(NN_THREADS) void chamfer_matrix_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                                    int qstride, int nq, const float* __restrict__ t,
                                                                    const int* __restrict__ toff, int tstride, int nt,
                                                                    const int* __restrict__ qb_start, int run, int runs,
                                                                    int tri, double* __restrict__ part) {
    __shared__ float4 tile[NN_TILE];
    __shared__ double sh[NN_THREADS / 64];
    const int tid = threadIdx.x;
    const int g = blockIdx.x / runs, r = blockIdx.x - g * runs;
    const int c = segment_of(qb_start, nq, g), qb = g - qb_start[c], nqb = qb_start[c + 1] - qb_start[c];
    int j0 = r * run, j1 = min(nt, j0 + run);
    if (tri > 0) j0 = max(j0, c + 1);
    if (tri < 0) j1 = min(j1, c);
    if (j0 >= j1) return;                                // (uniform over the workgroup)
    const int q0 = qoff[c], nqp = qoff[c + 1] - q0;

    const PackedQueries pq = load_queries(q, q0, nqp, qstride, qb, tid);

    for (int j = j0; j < j1; ++j) {
        const int t0 = toff[j], ntp = toff[j + 1] - t0;
        f2 best[NN_R / 2];
#pragma unroll
        for (int k = 0; k < NN_R / 2; ++k) best[k] = f2{INFINITY, INFINITY};
        for (int base = 0; base < ntp; base += NN_TILE) {
            const int n4 = stage_tile(tile, t, t0 + base, min(NN_TILE, ntp - base), tstride, tid);
            sweep_tile(tile, 0, n4, pq, best);
        }
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NN_R / 2; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (qb * NN_QB + (2 * k + h) * NN_THREADS + tid < nqp) acc += (double)(h ? best[k].y : best[k].x);
        }
        acc = block_sum(acc, sh);
        if (tid == 0) part[(size_t)qb_start[c] * nt + (size_t)j * nqb + qb] = acc;
    }
}

// one thread per (query cloud c, target cloud j): the block sums in block order, divided once.  main[c * mc + j * mj] gets the
// mean; in the symmetric case the other matrix's mirrored entry (mirror[c * mj + j * mc]) gets it too.
__global__ __launch_bounds__(256) void matrix_finish_kernel(const double* __restrict__ part, const int* __restrict__ qoff,
                                                            const int* __restrict__ qb_start, int nq, int nt, int tri,
                                                            double* __restrict__ main_out, long long mc, long long mj,
                                                            double* __restrict__ mirror) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)nq * nt) return;
    const int c = (int)(e / nt), j = (int)(e - (long long)c * nt);
    if ((tri > 0 && j <= c) || (tri < 0 && j >= c)) return;
    const int nqb = qb_start[c + 1] - qb_start[c];
    const double* p = part + (size_t)qb_start[c] * nt + (size_t)j * nqb;
    double s = 0.0;
    for (int b = 0; b < nqb; ++b) s += p[b];
    s /= (double)(qoff[c + 1] - qoff[c]);
    main_out[c * mc + j * mj] = s;
    if (mirror) mirror[c * mj + j * mc] = s;
}

// one workgroup per row: every thread scans its columns upwards (a strict < keeps the first), then the 256 candidates are
// merged pairwise with "smaller value, else smaller column" -- the lowest column attaining the row minimum, in any order
__global__ __launch_bounds__(256) void row_argmin_kernel(const double* __restrict__ m, int cols, int exclude_diag,
                                                         double* __restrict__ min_out, int* __restrict__ arg_out) {
    __shared__ double sv[256];
    __shared__ int si[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const double* p = m + (size_t)row * cols;
    double bv = INFINITY;
    int bi = 0x7fffffff;
    for (int j = tid; j < cols; j += 256) {
        if (exclude_diag && j == row) continue;
        const double v = p[j];
        if (v < bv || bi == 0x7fffffff) { bv = v; bi = j; }
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) {
            const double v = sv[tid + o];
            const int i = si[tid + o];
            if (v < sv[tid] || (v == sv[tid] && i < si[tid])) { sv[tid] = v; si[tid] = i; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        min_out[row] = sv[0];
        arg_out[row] = si[0] == 0x7fffffff ? -1 : si[0];
    }
}

// ---- range-image errors -------------------------------------------------------------------------------------------
constexpr int RE_MAXC = 8;
struct RangeErrArgs {                                    // kernel-argument block (not part of the C ABI)
    int chan[RE_MAXC];                                   // the selected channels, in order
    double scale[RE_MAXC], shift[RE_MAXC];               // per selected channel
    int nchan;
};

// one workgroup per image; window columns w0 + k (mod W) for k in [0, nw)
__global__ __launch_bounds__(1024) void range_errors_kernel(const float* __restrict__ a, const float* __restrict__ b, int C,
                                                            int W, int H, int w0, int nw, RangeErrArgs args,
                                                            double* __restrict__ abs_sum, double* __restrict__ sq_sum) {
    __shared__ double sh[16];
    const size_t img = (size_t)blockIdx.x * C * W * H;
    const int per_chan = nw * H, total = args.nchan * per_chan;
    double sa = 0.0, ss = 0.0;
    for (int e = threadIdx.x; e < total; e += 1024) {
        const int ci = e / per_chan, r = e - ci * per_chan;
        const int k = r / H, h = r - k * H;
        int w = w0 + k;
        if (w >= W) w -= W;
        const size_t o = img + ((size_t)args.chan[ci] * W + w) * H + h;
        const double s = args.scale[ci], t = args.shift[ci];
        const double d = ((double)a[o] * s + t) - ((double)b[o] * s + t);
        sa += fabs(d);
        ss += d * d;
    }
    sa = block_sum(sa, sh);
    ss = block_sum(ss, sh);
    if (threadIdx.x == 0) {
        abs_sum[blockIdx.x] = sa;
        sq_sum[blockIdx.x] = ss;
    }
}

// ---- beam upsampling ----------------------------------------------------------------------------------------------
// OpenCV's interpolateCubic (Keys, A = -0.75), fp32, in its operation order
__device__ inline void cubic_coeffs(float x, float c[4]) {
    const float A = -0.75f;
    c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// one thread per output pixel; rows are the contiguous beam axis of a (W, Hs) plane
__global__ __launch_bounds__(256) void beam_upsample_kernel(const float* __restrict__ src, int planes_w, int Hs, int rate,
                                                            int bicubic, double inv_rate, float* __restrict__ dst) {
    const int Hd = Hs * rate;
    const long long n = (long long)planes_w * Hd;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long line = e / Hd;
        const int r = (int)(e - line * Hd);
        const float* s = src + line * Hs;
        float v;
        if (!bicubic) {
            v = s[r / rate];                                             // INTER_NEAREST: floor(r / rate)
        } else {
            float fy = (float)(((double)r + 0.5) * inv_rate - 0.5);      // cv::resize: (dy + 0.5) * scale_y - 0.5
            const int sy = (int)floorf(fy);
            fy -= (float)sy;
            float c[4];
            cubic_coeffs(fy, c);
            float rows[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) rows[k] = s[min(max(sy - 1 + k, 0), Hs - 1)];   // replicated border
            v = ((c[0] * rows[0] + c[1] * rows[1]) + c[2] * rows[2]) + c[3] * rows[3];
        }
        dst[e] = v;
    }
}

}  // namespace

extern "C" {

int rldm_chamfer_nn(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                    int y_stride, int num_pairs, float* x_nn_d2, float* y_nn_d2, void* stream) {
    RLDM_REQUIRE(x && x_offsets && y && y_offsets && x_nn_d2 && y_nn_d2, "null argument");
    RLDM_REQUIRE(num_pairs > 0 && x_stride >= 3 && y_stride >= 3, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> xo(num_pairs + 1), yo(num_pairs + 1);
    if (int rc = fetch_offsets(st, x_offsets, xo, y_offsets, yo)) return rc;
    PairGrid wgs(st);                                    // [dir][num_pairs + 1]
    int splits[2];
    if (int rc = wgs.plan(xo, yo, NN_QB, NN_FILL_WGS, &splits[0])) return rc;
    if (int rc = wgs.plan(yo, xo, NN_QB, NN_FILL_WGS, &splits[1])) return rc;
    if (int rc = wgs.upload()) return rc;
    const int32_t* dstarts = wgs.dev.as<int32_t>();
    RLDM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(x_nn_d2), 0x7f800000, (size_t)xo[num_pairs], st));
    RLDM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(y_nn_d2), 0x7f800000, (size_t)yo[num_pairs], st));
    for (int dir = 0; dir < 2; ++dir) {
        const int grid = wgs.host[dir * (num_pairs + 1) + num_pairs];
        if (dir == 0)
            chamfer_nn_kernel<<<grid, NN_THREADS, 0, st>>>(x, x_offsets, x_stride, y, y_offsets, y_stride, num_pairs, dstarts,
                                                           splits[0], reinterpret_cast<unsigned*>(x_nn_d2));
        else
            chamfer_nn_kernel<<<grid, NN_THREADS, 0, st>>>(y, y_offsets, y_stride, x, x_offsets, x_stride, num_pairs,
                                                           dstarts + num_pairs + 1, splits[1],
                                                           reinterpret_cast<unsigned*>(y_nn_d2));
        RLDM_HIP_CHECK(hipGetLastError());
    }
    return wgs.finish();
}

int rldm_chamfer_mean(const float* x_nn_d2, const int32_t* x_offsets, const float* y_nn_d2, const int32_t* y_offsets,
                      int num_pairs, double* x_mean, double* y_mean, void* stream) {
    RLDM_REQUIRE(x_nn_d2 && x_offsets && y_nn_d2 && y_offsets && x_mean && y_mean, "null argument");
    RLDM_REQUIRE(num_pairs > 0, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    chamfer_mean_kernel<<<dim3(num_pairs, 2), 256, 0, st>>>(x_nn_d2, x_offsets, y_nn_d2, y_offsets, x_mean, y_mean);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_chamfer_matrix(const float* x, const int32_t* x_offsets, int x_stride, int nx, const float* y,
                        const int32_t* y_offsets, int y_stride, int ny, int symmetric, double* xy, double* yx, void* stream) {
    RLDM_REQUIRE(x && x_offsets && y && y_offsets && xy && yx, "null argument");
    RLDM_REQUIRE(nx > 0 && ny > 0 && x_stride >= 3 && y_stride >= 3, "bad shape");
    RLDM_REQUIRE(!symmetric || (x == y && x_offsets == y_offsets && x_stride == y_stride && nx == ny),
                 "symmetric: y must be x (the same buffers)");
    RLDM_REQUIRE((long long)nx * ny < (1LL << 31), "matrix too large (nx * ny must stay below 2^31)");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> off[2] = {std::vector<int32_t>(nx + 1), std::vector<int32_t>(ny + 1)};
    if (int rc = fetch_offsets(st, x_offsets, off[0], y_offsets, off[1])) return rc;
    const int n[2] = {nx, ny};
    // query-block tables of both sets in one allocation, [x: nx + 1][y: ny + 1]: the pair grid of a set against itself, unsplit
    PairGrid qbs(st);
    for (int s = 0; s < 2; ++s)
        if (int rc = qbs.plan(off[s], off[s], NN_QB, 0)) return rc;
    const int32_t* qb[2] = {qbs.host.data(), qbs.host.data() + nx + 1};
    // direction 0: X queries, Y targets; direction 1: Y queries, X targets.  A run is a whole number of target clouds: long
    // enough to amortise the query load (>= MX_RUN_POINTS targets on average), short enough that the grid has many more
    // workgroups than the chip has slots (the tail of an uneven last wave of workgroups stays small)
    constexpr long long MX_RUN_POINTS = 16384, MX_MAX_WGS = (1LL << 31) / NN_THREADS, MX_MAX_PART = 1LL << 28;
    int run[2], runs[2];
    long long part_len = 0;
    for (int d = 0; d < 2; ++d) {
        const int s = d, t = 1 - d;
        const long long blocks = qb[s][n[s]], tpoints = off[t][n[t]];
        RLDM_REQUIRE(blocks * n[t] <= MX_MAX_PART, "scratch too large (query blocks x target clouds above 2^28)");
        part_len = std::max(part_len, blocks * n[t]);
        const long long want = (16LL * NN_FILL_WGS + blocks - 1) / blocks;
        long long len = std::max<long long>((n[t] + want - 1) / want, (MX_RUN_POINTS * n[t] + tpoints - 1) / tpoints);
        len = std::min<long long>(std::max<long long>(len, 1), n[t]);
        while (len < n[t] && blocks * ((n[t] + len - 1) / len) >= MX_MAX_WGS) len *= 2;
        len = std::min<long long>(len, n[t]);
        run[d] = (int)len;
        runs[d] = (int)((n[t] + len - 1) / len);
        RLDM_REQUIRE(blocks * runs[d] < MX_MAX_WGS, "too many workgroups");
    }
    if (int rc = qbs.upload()) return rc;
    DevBuf pbuf(st);
    RLDM_HIP_CHECK(pbuf.alloc((size_t)part_len * sizeof(double)));
    const int32_t* dqb = qbs.dev.as<int32_t>();
    double* part = pbuf.as<double>();
    if (symmetric) {                                     // the diagonal; every other entry is written below
        RLDM_HIP_CHECK(hipMemsetAsync(xy, 0, (size_t)nx * ny * sizeof(double), st));
        RLDM_HIP_CHECK(hipMemsetAsync(yx, 0, (size_t)nx * ny * sizeof(double), st));
    }
    const int fin_grid = (int)(((long long)nx * ny + 255) / 256);
    for (int d = 0; d < 2; ++d) {                        // one after the other on the stream: they share `part`
        const int tri = symmetric ? (d ? -1 : 1) : 0;
        const int grid = qb[d][n[d]] * runs[d];
        if (d == 0) {
            chamfer_matrix_kernel<<<grid, NN_THREADS, 0, st>>>(x, x_offsets, x_stride, nx, y, y_offsets, y_stride, ny, dqb,
                                                               run[0], runs[0], tri, part);
            RLDM_HIP_CHECK(hipGetLastError());
            matrix_finish_kernel<<<fin_grid, 256, 0, st>>>(part, x_offsets, dqb, nx, ny, tri, xy, ny, 1,
                                                           symmetric ? yx : nullptr);
        } else {
            chamfer_matrix_kernel<<<grid, NN_THREADS, 0, st>>>(y, y_offsets, y_stride, ny, x, x_offsets, x_stride, nx,
                                                               dqb + nx + 1, run[1], runs[1], tri, part);
            RLDM_HIP_CHECK(hipGetLastError());
            matrix_finish_kernel<<<fin_grid, 256, 0, st>>>(part, y_offsets, dqb + nx + 1, ny, nx, tri, yx, 1, ny,
                                                           symmetric ? xy : nullptr);
        }
        RLDM_HIP_CHECK(hipGetLastError());
    }
    return qbs.finish();
}

int rldm_matrix_row_argmin(const double* m, int rows, int cols, int exclude_diag, double* min_out, int32_t* arg_out,
                           void* stream) {
    RLDM_REQUIRE(m && min_out && arg_out, "null argument");
    RLDM_REQUIRE(rows > 0 && cols > 0, "bad shape");
    row_argmin_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(m, cols, exclude_diag != 0, min_out, arg_out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_range_errors(const float* a, const float* b, int B, int C, int W, int H, int channel_mask, const float* scale,
                      const float* shift, int w0, int w1, double* abs_sum, double* sq_sum, void* stream) {
    RLDM_REQUIRE(a && b && scale && shift && abs_sum && sq_sum, "null argument");
    RLDM_REQUIRE(B > 0 && C > 0 && C <= RE_MAXC && W > 0 && H > 0, "bad shape (at most 8 channels)");
    RLDM_REQUIRE(channel_mask > 0 && channel_mask < (1 << C), "channel_mask must select channels of the image");
    RLDM_REQUIRE(w0 >= 0 && w0 < W && w1 > w0 && w1 <= w0 + W, "window must satisfy 0 <= w0 < W, w0 < w1 <= w0 + W");
    RLDM_REQUIRE((long long)C * W * H < (1LL << 31), "image too large");
    RangeErrArgs args{};
    for (int c = 0; c < C; ++c) {
        if (!(channel_mask >> c & 1)) continue;
        args.chan[args.nchan] = c;
        args.scale[args.nchan] = (double)scale[c];
        args.shift[args.nchan] = (double)shift[c];
        ++args.nchan;
    }
    hipStream_t st = (hipStream_t)stream;
    range_errors_kernel<<<B, 1024, 0, st>>>(a, b, C, W, H, w0, w1 - w0, args, abs_sum, sq_sum);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_beam_upsample(const float* src, int B, int C, int W, int Hs, int rate, int mode, float* dst, void* stream) {
    RLDM_REQUIRE(src && dst, "null argument");
    RLDM_REQUIRE(B > 0 && C > 0 && W > 0 && Hs > 0 && rate > 0, "bad shape");
    RLDM_REQUIRE(mode == RLDM_UPSAMPLE_NEAREST || mode == RLDM_UPSAMPLE_BICUBIC, "mode must be nearest (0) or bicubic (1)");
    hipStream_t st = (hipStream_t)stream;
    const long long lines = (long long)B * C * W;
    const long long n = lines * Hs * rate;
    const int grid = (int)std::min<long long>((n + 255) / 256, 256LL * 64);
    beam_upsample_kernel<<<grid, 256, 0, st>>>(src, (int)lines, Hs, rate, mode == RLDM_UPSAMPLE_BICUBIC, 1.0 / (double)rate,
                                               dst);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
