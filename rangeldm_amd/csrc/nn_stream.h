// nn_stream.h -- the brute-force nearest-neighbour stream that chamfer.hip, nn_index.hip and knn.hip share: its geometry, the
// query load, the LDS tile stage, the inner sweep, and the host plan of the (pair, query block, target chunk) grid.
//
// Numerics.  d^2 is computed directly as ((dx*dx + dy*dy) + dz*dz) with dx = xq - xt, every operation a single IEEE fp32
// rounding (no FMA contraction; packed v_pk_add_f32 / v_pk_mul_f32 round each half like the scalar op).  Every per-point
// minimum is therefore bit-equal to a CPU fp32 evaluation of the same expression, whatever the order in which the targets are
// visited, and the routes built on this header agree bit for bit.  The GEMM expansion |x|^2 + |y|^2 - 2 x.y (on the VALU or
// on the exact-f32 MFMA) is NOT used: at 70 m |x|^2 is about 4900 m^2, one fp32 ulp there is about 5e-4 m^2, larger than the
// typical nearest-neighbour d^2 of a dense scan -- the cancellation would leave no correct digit in the quantity being
// measured.  A file that includes this header carries `#pragma clang fp contract(off)` and is built with -ffp-contract=off
// (the Makefile's list), as eval_common.h says of its own inlines: the flag is what reaches the functions below.
//
// Structure.  A workgroup owns NN_QB = 256 x 8 query points of one cloud (8 per thread, held as 4 packed pairs in VGPRs) and
// streams target points past them through an LDS tile of NN_TILE points stored as float4; every lane reads the same tile
// entry at the same time (an LDS broadcast).  Tile entries past the end of the targets hold +inf coordinates: their d^2 is
// +inf and never wins.
#pragma once
#include "eval_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

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

// a lane's eight queries: query r is point qb * NN_QB + r * NN_THREADS + tid of its cloud, held in half r & 1 of pair r >> 1
struct PackedQueries {
    f2 x[NN_R / 2], y[NN_R / 2], z[NN_R / 2];
};

// the queries of block qb of the cloud of nq points that starts at packed point q0
__device__ __forceinline__ PackedQueries load_queries(const float* __restrict__ q, int q0, int nq, int qstride, int qb, int tid) {
    PackedQueries pq;
#pragma unroll
    for (int k = 0; k < NN_R / 2; ++k) {
        float v[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = min(qb * NN_QB + (2 * k + h) * NN_THREADS + tid, nq - 1);     // past the end: a valid duplicate
            const float* pt = q + (size_t)(q0 + i) * qstride;
            v[h][0] = pt[0]; v[h][1] = pt[1]; v[h][2] = pt[2];
        }
        pq.x[k] = f2{v[0][0], v[1][0]};
        pq.y[k] = f2{v[0][1], v[1][1]};
        pq.z[k] = f2{v[0][2], v[1][2]};
    }
    return pq;
}

// The n <= NN_TILE packed points from `first` on into the tile; with `pad`, +inf behind them up to the tile's end.  Both
// barriers are here: the one before the fill (the previous tile has been read) and the one after it.  Returns n rounded up
// to 4: with `pad`, entries [n, that) may be swept.  (knn.hip visits exactly n entries and asks for no padding.)
__device__ __forceinline__ int stage_tile(float4* tile, const float* __restrict__ t, int first, int n, int tstride, int tid,
                                          bool pad = true) {
    __syncthreads();
    for (int i = tid; i < (pad ? NN_TILE : n); i += NN_THREADS) {
        float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        if (i < n) {
            const float* pt = t + (size_t)(first + i) * tstride;
            v = make_float4(pt[0], pt[1], pt[2], 0.f);
        }
        tile[i] = v;
    }
    __syncthreads();
    return (n + 3) & ~3;
}

// lowers the four packed minima over the tile entries [j0, j1); j1 - j0 is a multiple of 4.  The queries come by value: by
// reference nn_index_kernel, which fills its 96 VGPRs, spills a query index around the stream
__device__ __forceinline__ void sweep_tile(const float4* tile, int j0, int j1, PackedQueries pq, f2 (&best)[NN_R / 2]) {
    for (int j = j0; j < j1; j += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 tp = tile[j + u];
            const f2 tx = f2{tp.x, tp.x}, ty = f2{tp.y, tp.y}, tz = f2{tp.z, tp.z};
#pragma unroll
            for (int k = 0; k < NN_R / 2; ++k) {
                const f2 dx = pq.x[k] - tx, dy = pq.y[k] - ty, dz = pq.z[k] - tz;
                const f2 d2 = (dx * dx + dy * dy) + dz * dz;
                best[k] = min2(best[k], d2);
            }
        }
    }
}

// Host side: the workgroup tables of a call, planned one after the other into one allocation.  A table has one entry per
// query cloud plus the total: wg_start[p] = first workgroup of pair p, where a pair takes (query blocks of `qblock` points) x
// (chunks of its target cloud).  Long target clouds are split so that a handful of pairs still fills the chip: into
// ceil(fill_wgs / query blocks of the call) chunks, no chunk shorter than a tile (pair_splits); fill_wgs = 0 never splits.
struct PairGrid {
    std::vector<int32_t> host;
    DevBuf dev;
    explicit PairGrid(hipStream_t st) : dev(st) {}

    // appends the table of one direction (as many entries as qo; its last is that direction's grid).  `splits` receives the
    // figure the kernel is given for pair_splits
    int plan(const std::vector<int32_t>& qo, const std::vector<int32_t>& to, int qblock, int fill_wgs, int* splits = nullptr) {
        const int n = (int)qo.size() - 1;
        long long qblocks = 0;
        for (int p = 0; p < n; ++p) qblocks += (qo[p + 1] - qo[p] + qblock - 1) / qblock;
        const int sp = (int)std::max<long long>(1, (fill_wgs + qblocks - 1) / qblocks);
        if (splits) *splits = sp;
        long long acc = 0;
        for (int p = 0; p < n; ++p) {
            host.push_back((int32_t)acc);
            const long long nqb = (qo[p + 1] - qo[p] + qblock - 1) / qblock;
            acc += nqb * pair_splits(sp, to[p + 1] - to[p]);
        }
        RLDM_REQUIRE(acc < (1LL << 31) / NN_THREADS, "too many workgroups");
        host.push_back((int32_t)acc);
        return 0;
    }
    // the planned tables on the device, in plan order
    int upload() {
        RLDM_HIP_CHECK(dev.alloc(host.size() * sizeof(int32_t)));
        RLDM_HIP_CHECK(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, dev.st));
        return 0;
    }
    // ends the call: `host` (pageable memory) must outlive its upload
    int finish() {
        RLDM_HIP_CHECK(hipStreamSynchronize(dev.st));
        return 0;
    }
};

}  // namespace
