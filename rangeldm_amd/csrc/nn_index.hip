// nn_index.hip -- the nearest neighbour WITH ITS INDEX, on gfx950: what chamfer.hip's chamfer_nn_kernel computes and throws
// away.  F-score at a distance threshold, Hausdorff distance, density-aware Chamfer distance and attribute transfer
// (rangeldm_amd/metrics.py) are all read off its outputs.
//
//   nn_index_kernel    for every query point the SQUARED distance to its nearest neighbour in the other cloud of its pair and
//                      the LOWEST index (local to that cloud) of a point at exactly that distance
//   nn_finish_kernel   unpacks the merged (d^2, index) keys where a target cloud was split, and counts per target point the
//                      queries that chose it (int32 atomics: exact, order-free)
//
// Numerics are chamfer.hip's (see its header): d^2 = ((dx*dx + dy*dy) + dz*dz), every operation one IEEE fp32 rounding, so
// each minimum has the bits rldm_chamfer_nn writes and the bits a CPU fp32 evaluation gives.
//
// Structure.  The streaming loop is chamfer_nn_kernel's: a workgroup owns 256 x 8 query points (4 packed pairs per thread)
// and one contiguous chunk of the target cloud, streamed through an LDS tile that every lane reads in step.  No index is
// carried through that loop.  Instead each thread compares its eight running minima once per NX_SUB = 64 target points,
// before against after, and remembers the LAST sub-block that strictly lowered each of them: that is the first sub-block that
// holds the final minimum (a later equal value does not lower it).  After the stream the thread re-reads that one sub-block
// per query from global memory (a different one per lane: cache traffic, not a broadcast), recomputes d^2 with the same
// expression and takes the lowest index whose d^2 has the minimum's bits (four queries at a time).  The check costs about 24 VALU instructions per
// sub-block against about 2 350 for the sub-block itself; the re-scan 64 evaluations per query against the whole chunk.
//
// A target cloud that one workgroup streams whole (splits == 1) writes d^2 and index directly.  Where clouds are split over
// workgroups (few pairs: fill the chip) the partial results are merged with one 64-bit atomicMin on
// (d^2 bits << 32) | index: non-negative floats order like their bit patterns, so the smallest d^2 wins and among equal d^2
// the lowest index.  Either way the result depends on the two clouds alone.
//
// Preconditions as rldm_chamfer_nn: clouds non-empty, coordinates finite.  NaN / inf coordinates give unspecified values,
// but every index written stays inside its cloud.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d^2 is three products and two sums, each rounded

namespace {

// the geometry of chamfer_nn_kernel (chamfer.hip keeps its own copy: that file is not touched by this one)
constexpr int NX_THREADS = 256;
constexpr int NX_R = 8;                       // query points per thread
constexpr int NX_QB = NX_THREADS * NX_R;      // query points per workgroup
constexpr int NX_TILE = 512;                  // target points per LDS tile (8 KiB)
constexpr int NX_SUB = 64;                    // target points between two looks at the running minima; divides NX_TILE
constexpr int NX_FILL_WGS = 256 * 8;          // split targets until about 8 workgroups per CU exist
constexpr int NX_NONE = 0x7fffffff;

typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

__device__ inline f2 min2(f2 a, f2 b) { return f2{fminf(a.x, b.x), fminf(a.y, b.y)}; }

// splits of one pair's target cloud: at most `splits`, and about a tile per chunk at least (host and device agree on this)
__host__ __device__ inline int pair_splits(int splits, int nt) {
    const int by_len = (nt + NX_TILE - 1) / NX_TILE;
    return splits < by_len ? splits : by_len;
}

// grid: one workgroup per (pair, query block, target chunk); wg_start[p] = first workgroup of pair p (num_pairs + 1 entries).
// keys != nullptr (pre-filled with all ones): atomicMin of (d^2 bits << 32 | local target index), indexed like the packed
// query array.  keys == nullptr (splits must be 1): d2_out / idx_out are written directly.  Five waves per SIMD: 96 VGPRs hold
// the loop's state (chamfer_nn_kernel's 64 plus eight saved minima and eight sub-block numbers) without scratch.
__global__ __launch_bounds__(NX_THREADS, 5) void nn_index_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                              int qstride, const float* __restrict__ t,
                                                              const int* __restrict__ toff, int tstride, int num_pairs,
                                                              const int* __restrict__ wg_start, int splits,
                                                              u64* __restrict__ keys, float* __restrict__ d2_out,
                                                              int* __restrict__ idx_out) {
    __shared__ float4 tile[NX_TILE];
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
    if (t_begin >= t_end) return;                        // an empty chunk has nothing to offer (uniform over the workgroup)

    f2 qx[NX_R / 2], qy[NX_R / 2], qz[NX_R / 2], best[NX_R / 2];
    int sub[NX_R];                                       // per query: the last sub-block of the chunk that lowered its minimum
#pragma unroll
    for (int k = 0; k < NX_R / 2; ++k) {
        float v[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = min(qb * NX_QB + (2 * k + h) * NX_THREADS + tid, nq - 1);     // past the end: a valid duplicate
            const float* pt = q + (size_t)(q0 + i) * qstride;
            v[h][0] = pt[0]; v[h][1] = pt[1]; v[h][2] = pt[2];
            sub[2 * k + h] = 0;
        }
        qx[k] = f2{v[0][0], v[1][0]};
        qy[k] = f2{v[0][1], v[1][1]};
        qz[k] = f2{v[0][2], v[1][2]};
        best[k] = f2{INFINITY, INFINITY};
    }

    for (int base = t_begin; base < t_end; base += NX_TILE) {
        const int n = min(NX_TILE, t_end - base);
        __syncthreads();                                 // the previous tile has been read
        for (int i = tid; i < NX_TILE; i += NX_THREADS) {
            float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            if (i < n) {
                const float* pt = t + (size_t)(t0 + base + i) * tstride;
                v = make_float4(pt[0], pt[1], pt[2], 0.f);
            }
            tile[i] = v;
        }
        __syncthreads();
        const int n4 = (n + 3) & ~3;                     // entries [n, n4) are the +inf padding
        for (int j0 = 0; j0 < n4; j0 += NX_SUB) {
            f2 prev[NX_R / 2];
#pragma unroll
            for (int k = 0; k < NX_R / 2; ++k) prev[k] = best[k];
            const int j1 = min(n4, j0 + NX_SUB);
            for (int j = j0; j < j1; j += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 tp = tile[j + u];
                    const f2 tx = f2{tp.x, tp.x}, ty = f2{tp.y, tp.y}, tz = f2{tp.z, tp.z};
#pragma unroll
                    for (int k = 0; k < NX_R / 2; ++k) {
                        const f2 dx = qx[k] - tx, dy = qy[k] - ty, dz = qz[k] - tz;
                        const f2 d2 = (dx * dx + dy * dy) + dz * dz;
                        best[k] = min2(best[k], d2);
                    }
                }
            }
            const int here = (base - t_begin + j0) / NX_SUB;     // tiles start at multiples of NX_TILE from t_begin
#pragma unroll
            for (int k = 0; k < NX_R / 2; ++k) {
                if (best[k].x < prev[k].x) sub[2 * k] = here;
                if (best[k].y < prev[k].y) sub[2 * k + 1] = here;
            }
        }
    }

    // the lowest index in each query's sub-block whose d^2 has the minimum's bits: four queries at a time (four independent
    // loads per step; all eight at once would double the kernel's registers for a part that is a few per cent of its work)
    int found[NX_R];
#pragma unroll
    for (int g = 0; g < NX_R; g += 4) {
#pragma unroll
        for (int r = g; r < g + 4; ++r) found[r] = NX_NONE;
#pragma unroll 1
        for (int e = 0; e < NX_SUB; ++e) {
#pragma unroll
            for (int r = g; r < g + 4; ++r) {
                const int j = min(t_begin + sub[r] * NX_SUB + e, t_end - 1);     // past the end: the last point again
                const float* pt = t + (size_t)(t0 + j) * tstride;
                const float x = (r & 1) ? qx[r >> 1].y : qx[r >> 1].x;
                const float y = (r & 1) ? qy[r >> 1].y : qy[r >> 1].x;
                const float z = (r & 1) ? qz[r >> 1].y : qz[r >> 1].x;
                const float dx = x - pt[0], dy = y - pt[1], dz = z - pt[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 == ((r & 1) ? best[r >> 1].y : best[r >> 1].x)) found[r] = min(found[r], j);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < NX_R; ++r) {
        const int i = qb * NX_QB + r * NX_THREADS + tid;
        if (i >= nq) continue;
        const float b = (r & 1) ? best[r >> 1].y : best[r >> 1].x;
        if (keys) {
            atomicMin(keys + q0 + i, ((u64)__float_as_uint(b) << 32) | (unsigned)found[r]);
        } else {
            d2_out[q0 + i] = b;
            idx_out[q0 + i] = found[r];
        }
    }
}

// one thread per query point of one direction.  keys != nullptr: the merged key is unpacked into d2 / idx first.  Then the
// query's choice is counted on the target side: hits[toff[p] + idx] += 1.  An index outside the cloud (only NaN / inf
// coordinates leave one) is replaced by 0, so nothing is ever written out of bounds.
__global__ __launch_bounds__(256) void nn_finish_kernel(const u64* __restrict__ keys, float* __restrict__ d2,
                                                        int* __restrict__ idx, const int* __restrict__ qoff,
                                                        const int* __restrict__ toff, int num_pairs,
                                                        int* __restrict__ hits) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= qoff[num_pairs]) return;
    int lo = 0, hi = num_pairs;                          // qoff[lo] <= i < qoff[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (qoff[mid] <= i) lo = mid; else hi = mid;
    }
    int j;
    if (keys) {
        const u64 k = keys[i];
        d2[i] = __uint_as_float((unsigned)(k >> 32));
        j = (int)(unsigned)(k & 0xffffffffu);
    } else {
        j = idx[i];
    }
    const int t0 = toff[lo], nt = toff[lo + 1] - t0;
    if ((unsigned)j >= (unsigned)nt) j = 0;
    idx[i] = j;
    atomicAdd(hits + t0 + j, 1);
}

}  // namespace

extern "C" {

int rldm_nn_index(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                  int y_stride, int num_pairs, float* x_nn_d2, int32_t* x_nn_idx, float* y_nn_d2, int32_t* y_nn_idx,
                  int32_t* x_hits, int32_t* y_hits, void* stream) {
    RLDM_REQUIRE(x && x_offsets && y && y_offsets && x_nn_d2 && x_nn_idx && y_nn_d2 && y_nn_idx && x_hits && y_hits,
                 "null argument");
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
        qblocks[0] += (xo[p + 1] - xo[p] + NX_QB - 1) / NX_QB;
        qblocks[1] += (yo[p + 1] - yo[p] + NX_QB - 1) / NX_QB;
    }
    RLDM_REQUIRE((long long)xo[num_pairs] + 255 < (1LL << 31) && (long long)yo[num_pairs] + 255 < (1LL << 31), "too many points");
    // workgroup tables of both directions in one allocation: [dir][num_pairs + 1] (rldm_chamfer_nn's split rule)
    std::vector<int32_t> starts(2 * (num_pairs + 1));
    int splits[2];
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int32_t>& qo = dir ? yo : xo;
        const std::vector<int32_t>& to = dir ? xo : yo;
        splits[dir] = (int)std::max<long long>(1, (NX_FILL_WGS + qblocks[dir] - 1) / qblocks[dir]);
        int32_t* ws = starts.data() + dir * (num_pairs + 1);
        long long acc = 0;
        for (int p = 0; p < num_pairs; ++p) {
            ws[p] = (int32_t)acc;
            const long long nqb = (qo[p + 1] - qo[p] + NX_QB - 1) / NX_QB;
            acc += nqb * pair_splits(splits[dir], to[p + 1] - to[p]);
        }
        RLDM_REQUIRE(acc < (1LL << 31) / NX_THREADS, "too many workgroups");
        ws[num_pairs] = (int32_t)acc;
    }
    const size_t nx = (size_t)xo[num_pairs], ny = (size_t)yo[num_pairs];
    // merge keys only for a direction whose target clouds are split: [x keys][y keys]
    const size_t kx = splits[0] > 1 ? nx : 0, ky = splits[1] > 1 ? ny : 0;
    DevBuf sbuf(st), kbuf(st);
    RLDM_HIP_CHECK(sbuf.alloc(starts.size() * sizeof(int32_t)));
    int32_t* dstarts = sbuf.as<int32_t>();
    RLDM_HIP_CHECK(hipMemcpyAsync(dstarts, starts.data(), starts.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    u64* keys[2] = {nullptr, nullptr};
    if (kx + ky) {
        RLDM_HIP_CHECK(kbuf.alloc((kx + ky) * sizeof(u64)));
        RLDM_HIP_CHECK(hipMemsetAsync(kbuf.p, 0xff, (kx + ky) * sizeof(u64), st));
        if (kx) keys[0] = kbuf.as<u64>();
        if (ky) keys[1] = kbuf.as<u64>() + kx;
    }
    RLDM_HIP_CHECK(hipMemsetAsync(x_hits, 0, nx * sizeof(int32_t), st));
    RLDM_HIP_CHECK(hipMemsetAsync(y_hits, 0, ny * sizeof(int32_t), st));
    for (int dir = 0; dir < 2; ++dir) {
        const int grid = starts[dir * (num_pairs + 1) + num_pairs];
        if (dir == 0) {
            nn_index_kernel<<<grid, NX_THREADS, 0, st>>>(x, x_offsets, x_stride, y, y_offsets, y_stride, num_pairs, dstarts,
                                                         splits[0], keys[0], x_nn_d2, x_nn_idx);
            RLDM_HIP_CHECK(hipGetLastError());
            nn_finish_kernel<<<(int)((nx + 255) / 256), 256, 0, st>>>(keys[0], x_nn_d2, x_nn_idx, x_offsets, y_offsets,
                                                                      num_pairs, y_hits);
        } else {
            nn_index_kernel<<<grid, NX_THREADS, 0, st>>>(y, y_offsets, y_stride, x, x_offsets, x_stride, num_pairs,
                                                         dstarts + num_pairs + 1, splits[1], keys[1], y_nn_d2, y_nn_idx);
            RLDM_HIP_CHECK(hipGetLastError());
            nn_finish_kernel<<<(int)((ny + 255) / 256), 256, 0, st>>>(keys[1], y_nn_d2, y_nn_idx, y_offsets, x_offsets,
                                                                      num_pairs, x_hits);
        }
        RLDM_HIP_CHECK(hipGetLastError());
    }
    RLDM_HIP_CHECK(hipStreamSynchronize(st));          // `starts` (pageable host memory) must outlive its upload
    return 0;
}

}  // extern "C"
