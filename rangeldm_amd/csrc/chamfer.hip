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
// Nearest-neighbour numerics.  d^2 is computed directly as ((dx*dx + dy*dy) + dz*dz) with dx = xq - xt, every operation a
// single IEEE fp32 rounding (no FMA contraction: -ffp-contract=off in the Makefile plus the pragma below; packed
// v_pk_add_f32 / v_pk_mul_f32 round each half like the scalar op).  Every per-point minimum is therefore bit-equal to a CPU
// fp32 evaluation of the same expression, whatever the order in which the targets are visited.  The GEMM expansion
// |x|^2 + |y|^2 - 2 x.y (on the VALU or on the exact-f32 MFMA) is NOT used: at 70 m |x|^2 is about 4900 m^2, one fp32 ulp
// there is about 5e-4 m^2, larger than the typical nearest-neighbour d^2 of a dense scan -- the cancellation would leave
// no correct digit in the quantity being measured.
//
// Structure.  A workgroup owns NN_QB = 256 x 8 query points of one pair (8 per thread, held as 4 packed pairs in VGPRs)
// and one contiguous chunk of that pair's target cloud, which it streams through an LDS tile of NN_TILE points stored as
// float4; every lane reads the same tile entry at the same time (an LDS broadcast).  Long target clouds are split over
// several workgroups so that a handful of pairs still fills the chip; the partial minima are merged with atomicMin on the
// bit pattern (non-negative floats order like uint32), so the result does not depend on the split.  Tile entries past the
// end of the chunk hold +inf coordinates: their d^2 is +inf and never wins.
//
// Preconditions: clouds are non-empty (the Python layer raises ValueError); coordinates are finite -- NaN or inf inputs
// give unspecified results (not checked).
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d^2 and the cubic weights are single IEEE ops

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_R = 8;                       // query points per thread
constexpr int NN_QB = NN_THREADS * NN_R;      // query points per workgroup
constexpr int NN_TILE = 512;                  // target points per LDS tile (8 KiB)
constexpr int NN_FILL_WGS = 256 * 8;          // split targets until about 8 workgroups per CU exist

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ inline f2 min2(f2 a, f2 b) { return f2{fminf(a.x, b.x), fminf(a.y, b.y)}; }

// splits of one pair's target cloud: at most `splits`, and no chunk shorter than a tile (host and device agree on this)
__host__ __device__ inline int pair_splits(int splits, int nt) {
    const int by_len = (nt + NN_TILE - 1) / NN_TILE;
    return splits < by_len ? splits : by_len;
}

// grid: one workgroup per (pair, query block, target chunk); wg_start[p] = first workgroup of pair p (num_pairs + 1 entries).
// out (pre-filled with +inf) receives atomicMin of the float bit patterns, indexed like the packed query array.
__global__ __launch_bounds__(NN_THREADS) void chamfer_nn_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                                int qstride, const float* __restrict__ t,
                                                                const int* __restrict__ toff, int tstride, int num_pairs,
                                                                const int* __restrict__ wg_start, int splits,
                                                                unsigned* __restrict__ out) {
    __shared__ float4 tile[NN_TILE];
    const int wg = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = num_pairs;                          // wg_start[lo] <= wg < wg_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wg_start[mid] <= wg) lo = mid; else hi = mid;
    }
    const int p = lo;
    const int q0 = qoff[p], nq = qoff[p + 1] - q0, t0 = toff[p], nt = toff[p + 1] - t0;
    const int sp = pair_splits(splits, nt);
    const int local = wg - wg_start[p];
    const int qb = local / sp, s = local - qb * sp;
    const int chunk = (nt + sp - 1) / sp;
    const int t_begin = s * chunk, t_end = min(nt, t_begin + chunk);

    f2 qx[NN_R / 2], qy[NN_R / 2], qz[NN_R / 2], best[NN_R / 2];
#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) {
        float v[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = min(qb * NN_QB + (2 * k + h) * NN_THREADS + tid, nq - 1);     // past the end: a valid duplicate
            const float* pt = q + (size_t)(q0 + i) * qstride;
            v[h][0] = pt[0]; v[h][1] = pt[1]; v[h][2] = pt[2];
        }
        qx[k] = f2{v[0][0], v[1][0]};
        qy[k] = f2{v[0][1], v[1][1]};
        qz[k] = f2{v[0][2], v[1][2]};
        best[k] = f2{INFINITY, INFINITY};
    }

    for (int base = t_begin; base < t_end; base += NN_TILE) {
        const int n = min(NN_TILE, t_end - base);
        __syncthreads();                                 // the previous tile has been read
        for (int i = tid; i < NN_TILE; i += NN_THREADS) {
            float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            if (i < n) {
                const float* pt = t + (size_t)(t0 + base + i) * tstride;
                v = make_float4(pt[0], pt[1], pt[2], 0.f);
            }
            tile[i] = v;
        }
        __syncthreads();
        const int n4 = (n + 3) & ~3;                     // entries [n, n4) are the +inf padding
        for (int j = 0; j < n4; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 tp = tile[j + u];
                const f2 tx = f2{tp.x, tp.x}, ty = f2{tp.y, tp.y}, tz = f2{tp.z, tp.z};
#pragma unroll
                for (int k = 0; k < NN_R / 2; ++k) {
                    const f2 dx = qx[k] - tx, dy = qy[k] - ty, dz = qz[k] - tz;
                    const f2 d2 = (dx * dx + dy * dy) + dz * dz;
                    best[k] = min2(best[k], d2);
                }
            }
        }
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
// (tri > 0) or below (tri < 0) the query cloud -- stream through the LDS tile with chamfer_nn_kernel's inner loop.  A target
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
    int lo = 0, hi = nq;                                 // qb_start[lo] <= g < qb_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (qb_start[mid] <= g) lo = mid; else hi = mid;
    }
    const int c = lo, qb = g - qb_start[c], nqb = qb_start[c + 1] - qb_start[c];
    int j0 = r * run, j1 = min(nt, j0 + run);
    if (tri > 0) j0 = max(j0, c + 1);
    if (tri < 0) j1 = min(j1, c);
    if (j0 >= j1) return;                                // (uniform over the workgroup)
    const int q0 = qoff[c], nqp = qoff[c + 1] - q0;

    f2 qx[NN_R / 2], qy[NN_R / 2], qz[NN_R / 2];
#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) {
        float v[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = min(qb * NN_QB + (2 * k + h) * NN_THREADS + tid, nqp - 1);    // past the end: a valid duplicate
            const float* pt = q + (size_t)(q0 + i) * qstride;
            v[h][0] = pt[0]; v[h][1] = pt[1]; v[h][2] = pt[2];
        }
        qx[k] = f2{v[0][0], v[1][0]};
        qy[k] = f2{v[0][1], v[1][1]};
        qz[k] = f2{v[0][2], v[1][2]};
    }

    for (int j = j0; j < j1; ++j) {
        const int t0 = toff[j], ntp = toff[j + 1] - t0;
        f2 best[NN_R / 2];
#pragma unroll
        for (int k = 0; k < NN_R / 2; ++k) best[k] = f2{INFINITY, INFINITY};
        for (int base = 0; base < ntp; base += NN_TILE) {
            const int n = min(NN_TILE, ntp - base);
            __syncthreads();                             // the previous tile has been read
            for (int i = tid; i < NN_TILE; i += NN_THREADS) {
                float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
                if (i < n) {
                    const float* pt = t + (size_t)(t0 + base + i) * tstride;
                    v = make_float4(pt[0], pt[1], pt[2], 0.f);
                }
                tile[i] = v;
            }
            __syncthreads();
            const int n4 = (n + 3) & ~3;                 // entries [n, n4) are the +inf padding
            for (int e = 0; e < n4; e += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 tp = tile[e + u];
                    const f2 tx = f2{tp.x, tp.x}, ty = f2{tp.y, tp.y}, tz = f2{tp.z, tp.z};
#pragma unroll
                    for (int k = 0; k < NN_R / 2; ++k) {
                        const f2 dx = qx[k] - tx, dy = qy[k] - ty, dz = qz[k] - tz;
                        const f2 d2 = (dx * dx + dy * dy) + dz * dz;
                        best[k] = min2(best[k], d2);
                    }
                }
            }
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
    RLDM_HIP_CHECK(hipMemcpyAsync(xo.data(), x_offsets, xo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipMemcpyAsync(yo.data(), y_offsets, yo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_REQUIRE(xo[0] == 0 && yo[0] == 0, "offsets must start at 0");
    long long qblocks[2] = {0, 0};
    for (int p = 0; p < num_pairs; ++p) {
        RLDM_REQUIRE(xo[p + 1] > xo[p] && yo[p + 1] > yo[p], "every cloud must be non-empty");
        qblocks[0] += (xo[p + 1] - xo[p] + NN_QB - 1) / NN_QB;
        qblocks[1] += (yo[p + 1] - yo[p] + NN_QB - 1) / NN_QB;
    }
    // workgroup tables of both directions in one allocation: [dir][num_pairs + 1]
    std::vector<int32_t> starts(2 * (num_pairs + 1));
    int splits[2];
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int32_t>& qo = dir ? yo : xo;
        const std::vector<int32_t>& to = dir ? xo : yo;
        splits[dir] = (int)std::max<long long>(1, (NN_FILL_WGS + qblocks[dir] - 1) / qblocks[dir]);
        int32_t* ws = starts.data() + dir * (num_pairs + 1);
        long long acc = 0;
        for (int p = 0; p < num_pairs; ++p) {
            ws[p] = (int32_t)acc;
            const long long nqb = (qo[p + 1] - qo[p] + NN_QB - 1) / NN_QB;
            acc += nqb * pair_splits(splits[dir], to[p + 1] - to[p]);
        }
        RLDM_REQUIRE(acc < (1LL << 31) / NN_THREADS, "too many workgroups");
        ws[num_pairs] = (int32_t)acc;
    }
    DevBuf dbuf(st);
    RLDM_HIP_CHECK(dbuf.alloc(starts.size() * sizeof(int32_t)));
    int32_t* dstarts = dbuf.as<int32_t>();
    RLDM_HIP_CHECK(hipMemcpyAsync(dstarts, starts.data(), starts.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RLDM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(x_nn_d2), 0x7f800000, (size_t)xo[num_pairs], st));
    RLDM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(y_nn_d2), 0x7f800000, (size_t)yo[num_pairs], st));
    for (int dir = 0; dir < 2; ++dir) {
        const int32_t* ws = starts.data() + dir * (num_pairs + 1);
        const int grid = ws[num_pairs];
        if (dir == 0)
            chamfer_nn_kernel<<<grid, NN_THREADS, 0, st>>>(x, x_offsets, x_stride, y, y_offsets, y_stride, num_pairs, dstarts,
                                                           splits[0], reinterpret_cast<unsigned*>(x_nn_d2));
        else
            chamfer_nn_kernel<<<grid, NN_THREADS, 0, st>>>(y, y_offsets, y_stride, x, x_offsets, x_stride, num_pairs,
                                                           dstarts + num_pairs + 1, splits[1],
                                                           reinterpret_cast<unsigned*>(y_nn_d2));
        RLDM_HIP_CHECK(hipGetLastError());
    }
    RLDM_HIP_CHECK(hipStreamSynchronize(st));          // `starts` (pageable host memory) must outlive its upload
    return 0;
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
    RLDM_HIP_CHECK(hipMemcpyAsync(off[0].data(), x_offsets, off[0].size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipMemcpyAsync(off[1].data(), y_offsets, off[1].size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_REQUIRE(off[0][0] == 0 && off[1][0] == 0, "offsets must start at 0");
    const int n[2] = {nx, ny};
    // query-block tables of both sets in one allocation: [x: nx + 1][y: ny + 1]
    std::vector<int32_t> qbs(nx + ny + 2);
    int32_t* qb[2] = {qbs.data(), qbs.data() + nx + 1};
    for (int s = 0; s < 2; ++s) {
        long long acc = 0;
        for (int c = 0; c < n[s]; ++c) {
            RLDM_REQUIRE(off[s][c + 1] > off[s][c], "every cloud must be non-empty");
            qb[s][c] = (int32_t)acc;
            acc += (off[s][c + 1] - off[s][c] + NN_QB - 1) / NN_QB;
        }
        qb[s][n[s]] = (int32_t)acc;
    }
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
    DevBuf qbuf(st), pbuf(st);
    RLDM_HIP_CHECK(qbuf.alloc(qbs.size() * sizeof(int32_t)));
    RLDM_HIP_CHECK(pbuf.alloc((size_t)part_len * sizeof(double)));
    int32_t* dqb = qbuf.as<int32_t>();
    double* part = pbuf.as<double>();
    RLDM_HIP_CHECK(hipMemcpyAsync(dqb, qbs.data(), qbs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
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
    RLDM_HIP_CHECK(hipStreamSynchronize(st));          // `qbs` (pageable host memory) must outlive its upload
    return 0;
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
