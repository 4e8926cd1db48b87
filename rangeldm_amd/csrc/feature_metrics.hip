// feature_metrics.hip -- row scans over the pairwise products of two activation sets, fp64 throughout, without ever forming
// an n_a x n_b matrix: what the kernel distance (KID's unbiased polynomial-kernel MMD^2) and precision /
// recall / density / coverage on k-nearest-neighbour manifolds (Kynkaanniemi et al. 2019, Naeem et al. 2020) reduce to.
//
//   g(a, b)   the dot product, K ascending in one fixed order without split-K: the tile of gram_f64.h, which fr_gram_kernel
//             (frechet.hip) stores, so g is the value rldm_gram_f64 gives
//   s(a)      g(a, a), from the same product path (fs_rownorm_kernel runs the diagonal MFMA tiles of x . x^T)
//   d2(a, b)  max(0, (s(a) + s(b)) - 2 g(a, b)), in that order: two identical rows are at exactly 0
//   kappa     t = g / d + 1; t * t * t
//
//   fs_rownorm_kernel    s(x_i): one wave per 16 rows runs their 16 x 16 diagonal tile of x . x^T and keeps its diagonal
//   fs_scan_kernel       workgroup (c, r) owns rows 64 r .. 64 r + 63 of A and streams the columns of chunk c of B past them
//                        in tiles of 64: products on v_mfma_f64_16x16x4_f64, the tile to LDS (over the operand stages, which
//                        are free by then), then one thread per row folds its 64 values, ascending j, into per-row state.
//                        No tile goes to global memory.
//   fs_merge_kernel      one thread per row combines the chunks in ascending order (only launched with more than one chunk)
//
// Column chunks: chunk_cols(n_b) = 64 * ceil(ceil(n_b / 64) / 16), a function of n_b alone, so at most 16 chunks and a
// row's outputs depend on that row and on B alone whatever the grid.  The k + 1 smallest values, integer counts and a
// minimum do not depend on the merge order; poly_sum is the sum, over ascending chunks, of each chunk's ascending-j sum.
//
// NaN / inf anywhere in an input: the call returns before anything else runs (eval_common.h's check_finite_f64).
#include "eval_common.h"
#include "gram_f64.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) (s_a + s_b) - 2 g and t * t * t are single IEEE ops

namespace {

constexpr int FS_THREADS = GR_THREADS;
constexpr int FS_TILE = GR_TILE;         // rows of A a workgroup owns; columns of B per tile
constexpr int FS_TLD = FS_TILE + 1;      // LDS row pitch of the product tile (f64)
constexpr int FS_LDS = GR_LDS;           // f64 in LDS: the tile's two operand stages, or (over them) one product tile
constexpr int FS_K1 = RLDM_FEATURE_MAX_K + 1;            // longest list of smallest values a row keeps
constexpr int FS_MAX_CHUNKS = 16;
constexpr int FS_MAX_ROWS = 65535 * FS_TILE;             // rows of A: one grid dimension of row blocks
static_assert(FS_TILE * FS_TLD <= FS_LDS, "the product tile must fit over the operand stages");

struct ScanArgs {
    const double* a; const double* b;    // [n_a][d], [n_b][d]
    const double* norm_a; const double* norm_b;
    const double* rad_a; const double* rad_b;            // [n_a], [n_b]; null: that count is not computed
    int n_a, n_b, d, k1, chunk_cols, poly, exclude_diagonal;
    long long row_offset;
    // per chunk c and row i, at c * n_a + i (kmin: times k1); null: not computed
    double* kmin; int* count_a; int* count_b; double* min_sq; double* poly_sum;
};

// norm[i] = g(x_i, x_i), one wave per 16 rows of a (the first blocks) or of b, straight from global memory.  In the f64 MFMA
// the A fragment of lane (r = lane & 15, q = lane >> 4) is x[r][k + q] and so is the B fragment, so one register feeds both
// operands; K is walked as gram_f64.h's tile walks it (ascending steps of 4 into one accumulator; its zero-filled steps add +0),
// so the diagonal of the 16 x 16 result is, bit for bit, what a tile holds for a row against itself.  Lane (r, q) holds
// result rows q + 4 reg of column r: the diagonal entry of row r sits in lane q == r & 3, reg r >> 2.
constexpr int FS_NORM_STEPS = 16;                        // MFMA steps (of 4 k) per round of loads

__global__ __launch_bounds__(64) void fs_rownorm_kernel(const double* a, int n_a, double* norm_a, const double* b, int n_b,
                                                       double* norm_b, int d) {
    const int blocks_a = (n_a + 15) / 16;
    const bool first = (int)blockIdx.x < blocks_a;
    const double* __restrict__ x = first ? a : b;
    double* __restrict__ norm = first ? norm_a : norm_b;
    const int n = first ? n_a : n_b;
    const int fr = threadIdx.x & 15, fk = threadIdx.x >> 4;
    const int row = ((int)blockIdx.x - (first ? 0 : blocks_a)) * 16 + fr;
    const bool valid = row < n;
    const double* __restrict__ xr = x + (size_t)(valid ? row : n - 1) * d;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 4 * FS_NORM_STEPS) {
        double v[FS_NORM_STEPS];
#pragma unroll
        for (int u = 0; u < FS_NORM_STEPS; ++u) {
            const int k = k0 + 4 * u + fk;
            v[u] = (valid && k < d) ? xr[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < FS_NORM_STEPS; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
    }
    if (!valid || fk != (fr & 3)) return;
    double s = acc[0];
#pragma unroll
    for (int reg = 1; reg < 4; ++reg)
        if (reg == (fr >> 2)) s = acc[reg];
    norm[row] = s;
}

// grid (chunks, ceil(n_a / 64))
__global__ __launch_bounds__(FS_THREADS, 4) void fs_scan_kernel(const ScanArgs p) {
    __shared__ double lds[FS_LDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, fr = lane & 15, fk = lane >> 4;
    const int i0 = blockIdx.y * FS_TILE;
    const int c0 = blockIdx.x * p.chunk_cols;
    const int c1 = min(c0 + p.chunk_cols, p.n_b);
    const int gi = i0 + t;                               // the row thread t < 64 folds
    const bool owner = t < FS_TILE && gi < p.n_a;
    const double dd = (double)p.d;
    const long long diag = (long long)gi + p.row_offset;

    double sa = 0.0, ra = 0.0;
    if (owner) {
        sa = p.norm_a[gi];
        if (p.rad_a) ra = p.rad_a[gi];
    }
    // the row's k1 smallest values so far live in its output row between tiles (ascending, inf until filled) and in registers
    // only while a tile is folded, when the accumulators are dead: the K loop keeps its occupancy
    double* const krow = p.kmin ? p.kmin + ((size_t)blockIdx.x * p.n_a + (owner ? gi : 0)) * p.k1 : nullptr;
    if (owner && krow)
        for (int i = 0; i < p.k1; ++i) krow[i] = INFINITY;
    double kth = INFINITY, mn = INFINITY, psum = 0.0;
    int ca = 0, cb = 0;

    for (int j0 = c0; j0 < c1; j0 += FS_TILE) {
        f64x4 acc[2][2];
        gram_tile_f64(p.a, p.n_a, i0, p.b, p.n_b, j0, p.d, lds, acc);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    lds[(wr + 16 * m + fk + 4 * reg) * FS_TLD + wc + 16 * n + fr] = acc[m][n][reg];
        __syncthreads();
        if (owner) {
            double list[FS_K1];                          // ascending; only the first k1 are kept right
#pragma unroll
            for (int i = 0; i < FS_K1; ++i) list[i] = (krow && i < p.k1) ? krow[i] : INFINITY;
            bool changed = false;
            const int cols = min(FS_TILE, c1 - j0);
            for (int j = 0; j < cols; ++j) {
                const double g = lds[t * FS_TLD + j];
                const double d2 = fmax(0.0, (sa + p.norm_b[j0 + j]) - 2.0 * g);
                mn = fmin(mn, d2);
                if (p.rad_a) ca += d2 < ra ? 1 : 0;
                if (p.rad_b) cb += d2 < p.rad_b[j0 + j] ? 1 : 0;
                if (p.poly && !(p.exclude_diagonal && (long long)(j0 + j) == diag)) {
                    const double tt = g / dd + 1.0;
                    psum += tt * tt * tt;
                }
                if (krow && d2 < kth) {                  // (kth is inf until k1 values are in: nothing is dropped early)
                    double v = d2;
#pragma unroll
                    for (int i = 0; i < FS_K1; ++i)
                        if (v < list[i]) { const double s = list[i]; list[i] = v; v = s; }
#pragma unroll
                    for (int i = 0; i < FS_K1; ++i)
                        if (i == p.k1 - 1) kth = list[i];
                    changed = true;
                }
            }
            if (changed) {
#pragma unroll
                for (int i = 0; i < FS_K1; ++i)
                    if (i < p.k1) krow[i] = list[i];
            }
        }
        __syncthreads();                                 // the next tile's operand stages overwrite the product tile
    }
    if (!owner) return;
    const size_t o = (size_t)blockIdx.x * p.n_a + gi;
    if (p.count_a) p.count_a[o] = ca;
    if (p.count_b) p.count_b[o] = cb;
    if (p.min_sq) p.min_sq[o] = mn;
    if (p.poly_sum) p.poly_sum[o] = psum;
}

// part: the per-chunk outputs of fs_scan_kernel; out: the same names, one chunk
struct MergeArgs {
    int n_a, k1, chunks;
    const double* kmin_p; const int* count_a_p; const int* count_b_p; const double* min_sq_p; const double* poly_sum_p;
    double* kmin; int* count_a; int* count_b; double* min_sq; double* poly_sum;
};

__global__ __launch_bounds__(FS_THREADS) void fs_merge_kernel(const MergeArgs p) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= p.n_a) return;
    if (p.kmin) {
        double list[FS_K1];
#pragma unroll
        for (int q = 0; q < FS_K1; ++q) list[q] = INFINITY;
        for (int c = 0; c < p.chunks; ++c)
            for (int e = 0; e < p.k1; ++e) {
                double v = p.kmin_p[((size_t)c * p.n_a + i) * p.k1 + e];
#pragma unroll
                for (int q = 0; q < FS_K1; ++q)
                    if (v < list[q]) { const double s = list[q]; list[q] = v; v = s; }
            }
#pragma unroll
        for (int q = 0; q < FS_K1; ++q)
            if (q < p.k1) p.kmin[(size_t)i * p.k1 + q] = list[q];
    }
    int ca = 0, cb = 0;
    double mn = INFINITY, ps = 0.0;
    for (int c = 0; c < p.chunks; ++c) {                 // ascending chunks: poly_sum's order
        const size_t o = (size_t)c * p.n_a + i;
        if (p.count_a) ca += p.count_a_p[o];
        if (p.count_b) cb += p.count_b_p[o];
        if (p.min_sq) mn = fmin(mn, p.min_sq_p[o]);
        if (p.poly_sum) ps += p.poly_sum_p[o];
    }
    if (p.count_a) p.count_a[i] = ca;
    if (p.count_b) p.count_b[i] = cb;
    if (p.min_sq) p.min_sq[i] = mn;
    if (p.poly_sum) p.poly_sum[i] = ps;
}

int chunk_cols(int n_b) {
    const int tiles = (n_b + FS_TILE - 1) / FS_TILE;
    return FS_TILE * ((tiles + FS_MAX_CHUNKS - 1) / FS_MAX_CHUNKS);
}

}  // namespace

extern "C" {

int rldm_feature_scan_column_chunk(int n_b) { return n_b > 0 ? chunk_cols(n_b) : 0; }

int rldm_feature_scan_f64(const double* a, int n_a, const double* b, int n_b, int d, int k1, const double* radius_sq_a,
                          const double* radius_sq_b, int poly, int exclude_diagonal, long long row_offset, double* kmin_sq,
                          int32_t* count_a, int32_t* count_b, double* min_sq, double* poly_sum, void* stream) {
    RLDM_REQUIRE(a && b, "null argument");
    RLDM_REQUIRE(n_a > 0 && n_b > 0 && d > 0, "bad shape");
    RLDM_REQUIRE(n_a <= FS_MAX_ROWS, "too many rows of a (a grid dimension holds 65535 blocks of 64 rows)");
    RLDM_REQUIRE(k1 >= 0 && k1 <= FS_K1, "k + 1 values per row can be kept for k up to RLDM_FEATURE_MAX_K");
    RLDM_REQUIRE((k1 > 0) == (kmin_sq != nullptr), "kmin_sq goes with k1 > 0");
    RLDM_REQUIRE(k1 <= n_b, "k1 smallest values need at least k1 rows of b");
    RLDM_REQUIRE((radius_sq_a != nullptr) == (count_a != nullptr), "count_a goes with radius_sq_a");
    RLDM_REQUIRE((radius_sq_b != nullptr) == (count_b != nullptr), "count_b goes with radius_sq_b");
    RLDM_REQUIRE((poly != 0) == (poly_sum != nullptr), "poly_sum goes with poly");
    RLDM_REQUIRE(row_offset >= 0, "row_offset must not be negative");
    hipStream_t st = (hipStream_t)stream;
    const bool self = a == b && n_a == n_b;
    const size_t na = (size_t)n_a, nb = (size_t)n_b;

    // NaN / inf anywhere: refused before anything else runs
    if (int rc = rldm::check_finite_f64({{a, na * d}, {self ? nullptr : b, nb * d}, {radius_sq_a, na}, {radius_sq_b, nb}}, st))
        return rc;

    const int cc = chunk_cols(n_b);
    const int chunks = (n_b + cc - 1) / cc;
    const bool merge = chunks > 1;
    // workspace: the row norms, and with more than one chunk the per-chunk outputs (at most 16 x what the caller gets)
    const size_t per = merge ? (size_t)chunks * na : 0;
    const size_t f64s = na + (self ? 0 : nb) + (kmin_sq ? per * k1 : 0) + (min_sq ? per : 0) + (poly_sum ? per : 0);
    const size_t i32s = (count_a ? per : 0) + (count_b ? per : 0);
    DevBuf buf(st);
    RLDM_HIP_CHECK(buf.alloc(f64s * sizeof(double) + i32s * sizeof(int)));
    double* w = buf.as<double>();
    double* norm_a = w; w += na;
    double* norm_b = self ? norm_a : w; w += self ? 0 : nb;
    ScanArgs s{};
    s.a = a; s.b = b; s.norm_a = norm_a; s.norm_b = norm_b; s.rad_a = radius_sq_a; s.rad_b = radius_sq_b;
    s.n_a = n_a; s.n_b = n_b; s.d = d; s.k1 = k1; s.chunk_cols = cc; s.poly = poly ? 1 : 0;
    s.exclude_diagonal = exclude_diagonal ? 1 : 0; s.row_offset = row_offset;
    s.kmin = kmin_sq; s.count_a = count_a; s.count_b = count_b; s.min_sq = min_sq; s.poly_sum = poly_sum;
    if (merge) {
        if (kmin_sq) { s.kmin = w; w += per * k1; }
        if (min_sq) { s.min_sq = w; w += per; }
        if (poly_sum) { s.poly_sum = w; w += per; }
        int* wi = reinterpret_cast<int*>(w);
        if (count_a) { s.count_a = wi; wi += per; }
        if (count_b) { s.count_b = wi; wi += per; }
    }

    fs_rownorm_kernel<<<(n_a + 15) / 16 + (self ? 0 : (n_b + 15) / 16), 64, 0, st>>>(a, n_a, norm_a, b, self ? 0 : n_b, norm_b, d);
    fs_scan_kernel<<<dim3(chunks, (n_a + FS_TILE - 1) / FS_TILE), FS_THREADS, 0, st>>>(s);
    if (merge) {
        MergeArgs m{};
        m.n_a = n_a; m.k1 = k1; m.chunks = chunks;
        m.kmin_p = s.kmin; m.count_a_p = s.count_a; m.count_b_p = s.count_b; m.min_sq_p = s.min_sq; m.poly_sum_p = s.poly_sum;
        m.kmin = kmin_sq; m.count_a = count_a; m.count_b = count_b; m.min_sq = min_sq; m.poly_sum = poly_sum;
        fs_merge_kernel<<<(n_a + FS_THREADS - 1) / FS_THREADS, FS_THREADS, 0, st>>>(m);
    }
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
