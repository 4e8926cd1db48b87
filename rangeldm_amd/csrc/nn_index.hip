// nn_index.hip -- the nearest neighbour WITH ITS INDEX, on gfx950: what chamfer.hip's chamfer_nn_kernel computes and throws
// away.  F-score at a distance threshold, Hausdorff distance, density-aware Chamfer distance and attribute transfer
// (rangeldm_amd/metrics.py) are all read off its outputs.
//
//   nn_index_kernel    for every query point the SQUARED distance to its nearest neighbour in the other cloud of its pair and
//                      the LOWEST index (local to that cloud) of a point at exactly that distance
//   nn_finish_kernel   unpacks the merged (d^2, index) keys where a target cloud was split, and counts per target point the
//                      queries that chose it (int32 atomics: exact, order-free)
//
// Numerics are nn_stream.h's (see its header): d^2 = ((dx*dx + dy*dy) + dz*dz), every operation one IEEE fp32 rounding, so
// each minimum has the bits rldm_chamfer_nn writes and the bits a CPU fp32 evaluation gives.
//
// Structure.  The streaming loop is nn_stream.h's, shared with chamfer_nn_kernel: a workgroup owns 256 x 8 query points (4
// packed pairs per thread) and one contiguous chunk of the target cloud, streamed through an LDS tile that every lane reads
// in step.  No index is carried through that loop.  Instead each thread compares its eight running minima once per
// NX_SUB = 64 target points, before against after, and remembers the LAST sub-block that strictly lowered each of them: that
// is the first sub-block that holds the final minimum (a later equal value does not lower it).  After the stream the thread
// re-reads that one sub-block per query from global memory (a different one per lane: cache traffic, not a broadcast),
// recomputes d^2 with the same expression and takes the lowest index whose d^2 has the minimum's bits (four queries at a
// time).  The check costs about 24 VALU instructions per sub-block against about 2 350 for the sub-block itself; the re-scan
// 64 evaluations per query against the whole chunk.
//
// A target cloud that one workgroup streams whole (splits == 1) writes d^2 and index directly.  Where clouds are split over
// workgroups (few pairs: fill the chip) the partial results are merged with one 64-bit atomicMin on
// (d^2 bits << 32) | index: non-negative floats order like their bit patterns, so the smallest d^2 wins and among equal d^2
// the lowest index.  Either way the result depends on the two clouds alone.
//
// Preconditions as rldm_chamfer_nn: clouds non-empty, coordinates finite.  NaN / inf coordinates give unspecified values,
// but every index written stays inside its cloud.
#include "nn_stream.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d^2 is three products and two sums, each rounded

namespace {

constexpr int NX_SUB = 64;                    // target points between two looks at the running minima; divides NN_TILE
constexpr int NX_NONE = 0x7fffffff;

typedef unsigned long long u64;

// grid: one workgroup per (pair, query block, target chunk); wg_start[p] = first workgroup of pair p (num_pairs + 1 entries).
// keys != nullptr (pre-filled with all ones): atomicMin of (d^2 bits << 32 | local target index), indexed like the packed
// query array.  keys == nullptr (splits must be 1): d2_out / idx_out are written directly.  Five waves per SIMD: 96 VGPRs hold
// the loop's state (chamfer_nn_kernel's 64 plus eight saved minima and eight sub-block numbers) without scratch.
__global__ __launch_bounds__(NN_THREADS, 5) void nn_index_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                              int qstride, const float* __restrict__ t,
                                                              const int* __restrict__ toff, int tstride, int num_pairs,
                                                              const int* __restrict__ wg_start, int splits,
                                                              u64* __restrict__ keys, float* __restrict__ d2_out,
                                                              int* __restrict__ idx_out) {
    __shared__ float4 tile[NN_TILE];
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int p = segment_of(wg_start, num_pairs, wg);
    const int q0 = qoff[p], nq = qoff[p + 1] - q0, t0 = toff[p], nt = toff[p + 1] - t0;
    const int sp = pair_splits(splits, nt);
    const int local = wg - wg_start[p];
    const int qb = local / sp, s = local - qb * sp;
    const int chunk = (nt + sp - 1) / sp;
    const int t_begin = s * chunk, t_end = min(nt, t_begin + chunk);
    if (t_begin >= t_end) return;                        // an empty chunk has nothing to offer (uniform over the workgroup)

    const PackedQueries pq = load_queries(q, q0, nq, qstride, qb, tid);
    f2 best[NN_R / 2];
    int sub[NN_R];                                       // per query: the last sub-block of the chunk that lowered its minimum
#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) {
        best[k] = f2{INFINITY, INFINITY};
        sub[2 * k] = sub[2 * k + 1] = 0;
    }

    for (int base = t_begin; base < t_end; base += NN_TILE) {
        const int n4 = stage_tile(tile, t, t0 + base, min(NN_TILE, t_end - base), tstride, tid);
        for (int j0 = 0; j0 < n4; j0 += NX_SUB) {
            f2 prev[NN_R / 2];
#pragma unroll
            for (int k = 0; k < NN_R / 2; ++k) prev[k] = best[k];
            sweep_tile(tile, j0, min(n4, j0 + NX_SUB), pq, best);
            const int here = (base - t_begin + j0) / NX_SUB;     // tiles start at multiples of NN_TILE from t_begin
#pragma unroll
            for (int k = 0; k < NN_R / 2; ++k) {
                if (best[k].x < prev[k].x) sub[2 * k] = here;
                if (best[k].y < prev[k].y) sub[2 * k + 1] = here;
            }
        }
    }

    // the lowest index in each query's sub-block whose d^2 has the minimum's bits: four queries at a time (four independent
    // loads per step; all eight at once would double the kernel's registers for a part that is a few per cent of its work)
    int found[NN_R];
#pragma unroll
    for (int g = 0; g < NN_R; g += 4) {
#pragma unroll
        for (int r = g; r < g + 4; ++r) found[r] = NX_NONE;
#pragma unroll 1
        for (int e = 0; e < NX_SUB; ++e) {
#pragma unroll
            for (int r = g; r < g + 4; ++r) {
                const int j = min(t_begin + sub[r] * NX_SUB + e, t_end - 1);     // past the end: the last point again
                const float* pt = t + (size_t)(t0 + j) * tstride;
                const float x = (r & 1) ? pq.x[r >> 1].y : pq.x[r >> 1].x;
                const float y = (r & 1) ? pq.y[r >> 1].y : pq.y[r >> 1].x;
                const float z = (r & 1) ? pq.z[r >> 1].y : pq.z[r >> 1].x;
                const float dx = x - pt[0], dy = y - pt[1], dz = z - pt[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 == ((r & 1) ? best[r >> 1].y : best[r >> 1].x)) found[r] = min(found[r], j);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < NN_R; ++r) {
        const int i = qb * NN_QB + r * NN_THREADS + tid;
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
    const int lo = segment_of(qoff, num_pairs, i);
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
    if (int rc = fetch_offsets(st, x_offsets, xo, y_offsets, yo)) return rc;
    RLDM_REQUIRE((long long)xo[num_pairs] + 255 < (1LL << 31) && (long long)yo[num_pairs] + 255 < (1LL << 31), "too many points");
    PairGrid wgs(st);                                    // [dir][num_pairs + 1], rldm_chamfer_nn's plan
    int splits[2];
    if (int rc = wgs.plan(xo, yo, NN_QB, NN_FILL_WGS, &splits[0])) return rc;
    if (int rc = wgs.plan(yo, xo, NN_QB, NN_FILL_WGS, &splits[1])) return rc;
    const size_t nx = (size_t)xo[num_pairs], ny = (size_t)yo[num_pairs];
    // merge keys only for a direction whose target clouds are split: [x keys][y keys]
    const size_t kx = splits[0] > 1 ? nx : 0, ky = splits[1] > 1 ? ny : 0;
    if (int rc = wgs.upload()) return rc;
    const int32_t* dstarts = wgs.dev.as<int32_t>();
    DevBuf kbuf(st);
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
        const int grid = wgs.host[dir * (num_pairs + 1) + num_pairs];
        if (dir == 0) {
            nn_index_kernel<<<grid, NN_THREADS, 0, st>>>(x, x_offsets, x_stride, y, y_offsets, y_stride, num_pairs, dstarts,
                                                         splits[0], keys[0], x_nn_d2, x_nn_idx);
            RLDM_HIP_CHECK(hipGetLastError());
            nn_finish_kernel<<<(int)((nx + 255) / 256), 256, 0, st>>>(keys[0], x_nn_d2, x_nn_idx, x_offsets, y_offsets,
                                                                      num_pairs, y_hits);
        } else {
            nn_index_kernel<<<grid, NN_THREADS, 0, st>>>(y, y_offsets, y_stride, x, x_offsets, x_stride, num_pairs,
                                                         dstarts + num_pairs + 1, splits[1], keys[1], y_nn_d2, y_nn_idx);
            RLDM_HIP_CHECK(hipGetLastError());
            nn_finish_kernel<<<(int)((ny + 255) / 256), 256, 0, st>>>(keys[1], y_nn_d2, y_nn_idx, y_offsets, x_offsets,
                                                                      num_pairs, x_hits);
        }
        RLDM_HIP_CHECK(hipGetLastError());
    }
    return wgs.finish();
}

}  // extern "C"
