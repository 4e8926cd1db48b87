// gram_f64.h -- the fp64 MFMA tile of rows of a times rows of b, stated once: fr_gram_kernel (frechet.hip) stores it,
// fs_scan_kernel (feature_metrics.hip) folds it.  Both run this one loop, so an entry of a scan's tile IS the value
// rldm_gram_f64 gives for its two rows, bit for bit (tests/test_feature_metrics_gpu.py holds the scan to it).
//
// f64 MFMA layout (NOT the one the f32-accumulator shapes share): A / B one f64 per lane, row (of A) or column (of B)
// lane & 15, k = lane >> 4; C / D four f64 per lane, column lane & 15, row (lane >> 4) + 4 * reg.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int GR_THREADS = 256;          // 4 waves
constexpr int GR_TILE = 64;              // output tile of a workgroup: 4 waves x (32 x 32)
constexpr int GR_BK = 32;                // K per LDS stage
constexpr int GR_LD = GR_BK + 1;         // LDS row pitch of an operand stage (f64)
constexpr int GR_LDS = 2 * GR_TILE * GR_LD;              // f64 in LDS: the two operand stages

// acc = rows i0 .. i0 + 63 of a times rows j0 .. j0 + 63 of b, transposed: K ascending in steps of 32 through LDS (lds holds
// GR_LDS doubles), zero filled at every edge, no split-K, so an entry depends on its two rows alone.  Wave w owns the 32 x 32
// block (w >> 1, w & 1) as 2 x 2 MFMA tiles: acc[m][n][reg] is row (w >> 1) * 32 + 16 m + (lane >> 4) + 4 reg, column
// (w & 1) * 32 + 16 n + (lane & 15).  Ends behind a barrier: LDS is free when it returns.
__device__ __forceinline__ void gram_tile_f64(const double* __restrict__ a, int n_a, int i0, const double* __restrict__ b,
                                              int n_b, int j0, int d, double* __restrict__ lds, f64x4 (&acc)[2][2]) {
    double* __restrict__ As = lds;
    double* __restrict__ Bs = lds + GR_TILE * GR_LD;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int lk = t & 31, lr = t >> 5;                  // loader: 32 consecutive k of 8 rows per pass
    const int fr = lane & 15, fk = lane >> 4;            // fragment: row (column) and k of this lane
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += GR_BK) {
        const int k = k0 + lk;
#pragma unroll
        for (int p = 0; p < GR_TILE / 8; ++p) {
            const int r = lr + 8 * p;
            const int gi = i0 + r, gj = j0 + r;
            As[r * GR_LD + lk] = (gi < n_a && k < d) ? a[(size_t)gi * d + k] : 0.0;
            Bs[r * GR_LD + lk] = (gj < n_b && k < d) ? b[(size_t)gj * d + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GR_BK; kk += 4) {
            double af[2], bf[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) af[m] = As[(wr + 16 * m + fr) * GR_LD + kk + fk];
#pragma unroll
            for (int n = 0; n < 2; ++n) bf[n] = Bs[(wc + 16 * n + fr) * GR_LD + kk + fk];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
    }
}

}  // namespace
