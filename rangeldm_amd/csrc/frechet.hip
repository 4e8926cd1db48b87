// frechet.hip -- the Frechet distance between Gaussians fitted to two sets of dumped activations (the reference's
// `metric.py --fid --fid_folder1 A --fid_folder2 B`), fp64 throughout, without ever forming a d x d matrix.
//
// With A (n1 x d), B (n2 x d) the centred activations, C1 = A^T A / (n1 - 1), C2 = B^T B / (n2 - 1):
//     Tr sqrtm(C1 C2) = |A B^T|_* / sqrt((n1 - 1)(n2 - 1))          (the non-zero eigenvalues of A^T A B^T B are the squared
//     Tr C1 = sum A^2 / (n1 - 1)                                      singular values of A B^T)
//
//   fr_finite_kernel        NaN / inf anywhere in an input: the call returns before anything else runs (the library's one
//                           finite check, rldm::check_finite_f64 of eval_common.h; feature_metrics.hip calls it too)
//   fr_colmean_kernel       column means, samples summed in ascending order (one thread per column)
//   fr_center_kernel        A = X - mean and per-row sum A^2 (one workgroup per row, fixed-order tree)
//   fr_totals_kernel        sum A^2, sum B^2, |mu1 - mu2|^2 (one workgroup, fixed-order trees)
//   fr_gram_kernel          M = A . B^T on v_mfma_f64_16x16x4_f64: the tile of gram_f64.h (64 x 64 per workgroup, K ascending
//                           in steps of 32 through LDS, no split-K), stored
//   fr_jacobi_step_kernel   one step of a one-sided (Hestenes) Jacobi sweep: one workgroup per column pair of the round-robin
//                           schedule.  The pairs of a step are disjoint, so no workgroup reads what another writes; the next
//                           step is the next launch.  Nothing in here waits on another workgroup or loops on convergence: the
//                           host counts sweeps and gives up at its cap.
//   fr_colnorm_kernel       the singular values: the final column norms
#include "eval_common.h"
#include "gram_f64.h"
#include "../../include/rangeldm_hip.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

namespace {

constexpr int FR_THREADS = GR_THREADS;                   // every kernel here, the tile's among them
constexpr int GR_MAX_ROWS = 65535 * GR_TILE;             // rows of either operand: one grid dimension of tiles

thread_local int fr_last_sweeps = 0;

// sum of one value per thread over the workgroup, the same tree every time; every thread gets the result.  (Not
// eval_common.h's block_sum: an LDS tree adds in another order, and the Frechet distance's last bits are this order's.)
__device__ __forceinline__ double block_sum_fixed(double v, double* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = FR_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(FR_THREADS) void fr_finite_kernel(const double* __restrict__ x, size_t n, int* __restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * FR_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * FR_THREADS)
        bad |= !__builtin_isfinite(x[i]);
    if (bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(FR_THREADS) void fr_colmean_kernel(const double* __restrict__ x, int n, int d,
                                                               double* __restrict__ mean) {
    const int j = blockIdx.x * FR_THREADS + threadIdx.x;
    if (j >= d) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[(size_t)i * d + j];
    mean[j] = s / (double)n;
}

__global__ __launch_bounds__(FR_THREADS) void fr_center_kernel(const double* __restrict__ x, const double* __restrict__ mean,
                                                              int d, double* __restrict__ a, double* __restrict__ rowsq) {
    __shared__ double lds[FR_THREADS];
    const size_t row = (size_t)blockIdx.x * d;
    double s = 0.0;
    for (int j = threadIdx.x; j < d; j += FR_THREADS) {
        const double v = x[row + j] - mean[j];
        a[row + j] = v;
        s += v * v;
    }
    s = block_sum_fixed(s, lds);
    if (threadIdx.x == 0) rowsq[blockIdx.x] = s;
}

// out3 = {sum rowsq1, sum rowsq2, |mu1 - mu2|^2}
__global__ __launch_bounds__(FR_THREADS) void fr_totals_kernel(const double* __restrict__ rowsq1, int n1,
                                                              const double* __restrict__ rowsq2, int n2,
                                                              const double* __restrict__ mu1, const double* __restrict__ mu2,
                                                              int d, double* __restrict__ out3) {
    __shared__ double lds[FR_THREADS];
    double s1 = 0.0, s2 = 0.0, sm = 0.0;
    for (int i = threadIdx.x; i < n1; i += FR_THREADS) s1 += rowsq1[i];
    for (int i = threadIdx.x; i < n2; i += FR_THREADS) s2 += rowsq2[i];
    for (int j = threadIdx.x; j < d; j += FR_THREADS) {
        const double v = mu1[j] - mu2[j];
        sm += v * v;
    }
    s1 = block_sum_fixed(s1, lds);
    s2 = block_sum_fixed(s2, lds);
    sm = block_sum_fixed(sm, lds);
    if (threadIdx.x == 0) {
        out3[0] = s1;
        out3[1] = s2;
        out3[2] = sm;
    }
}

// grid (ceil(n2 / 64), ceil(n1 / 64)); wave w owns the 32 x 32 block (w >> 1, w & 1) of the tile as 2 x 2 MFMA tiles
__global__ __launch_bounds__(FR_THREADS) void fr_gram_kernel(const double* __restrict__ a, int n1, const double* __restrict__ b,
                                                            int n2, int d, double* __restrict__ out) {
    __shared__ double lds[GR_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.y * GR_TILE, j0 = blockIdx.x * GR_TILE;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32, fr = lane & 15, fk = lane >> 4;
    f64x4 acc[2][2];
    gram_tile_f64(a, n1, i0, b, n2, j0, d, lds, acc);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = i0 + wr + 16 * m + fk + 4 * reg;
                const int gj = j0 + wc + 16 * n + fr;
                if (gi < n1 && gj < n2) out[(size_t)gi * n2 + gj] = acc[m][n][reg];
            }
}

// w [cols][rows] = m [rows][cols]^T
__global__ __launch_bounds__(FR_THREADS) void fr_transpose_kernel(const double* __restrict__ m, int rows, int cols,
                                                                 double* __restrict__ w) {
    const size_t total = (size_t)rows * cols;
    for (size_t o = (size_t)blockIdx.x * FR_THREADS + threadIdx.x; o < total; o += (size_t)gridDim.x * FR_THREADS) {
        const size_t j = o / rows, i = o - j * rows;
        w[o] = m[i * cols + j];
    }
}

// w: c columns of `len` contiguous values.  Step `step` (0 .. cpad - 2) of the round-robin schedule over cpad = c rounded up
// to even players: workgroup 0 plays (cpad - 1, step), workgroup b plays (step + b, step - b) mod (cpad - 1).  cpad - 1 is
// odd, so the cpad / 2 pairs of a step are disjoint and cover every player once.  Player c (the pad, when c is odd) has no
// column: its pair is skipped.
__global__ __launch_bounds__(FR_THREADS) void fr_jacobi_step_kernel(double* __restrict__ w, int c, int len, int cpad, int step,
                                                                   double tol, unsigned* __restrict__ rotations) {
    __shared__ double lds[FR_THREADS];
    const int m = cpad - 1, b = blockIdx.x;
    int p = b == 0 ? m : (step + b) % m;
    int q = b == 0 ? step : (step + m - b) % m;
    if (p > q) { const int s = p; p = q; q = s; }
    if (q >= c) return;
    double* __restrict__ ap = w + (size_t)p * len;
    double* __restrict__ aq = w + (size_t)q * len;
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
    for (int e = threadIdx.x; e < len; e += FR_THREADS) {
        const double x = ap[e], y = aq[e];
        alpha += x * x;
        beta += y * y;
        gamma += x * y;
    }
    alpha = block_sum_fixed(alpha, lds);
    beta = block_sum_fixed(beta, lds);
    gamma = block_sum_fixed(gamma, lds);
    if (alpha == 0.0 || beta == 0.0) return;
    if (fabs(gamma) <= tol * (sqrt(alpha) * sqrt(beta))) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
    if (sn == 0.0) return;                               // zeta overflowed (norms apart beyond fp64's range): nothing to apply
    for (int e = threadIdx.x; e < len; e += FR_THREADS) {
        const double x = ap[e], y = aq[e];
        ap[e] = cs * x - sn * y;
        aq[e] = sn * x + cs * y;
    }
    if (threadIdx.x == 0) atomicAdd(rotations, 1u);
}

__global__ __launch_bounds__(FR_THREADS) void fr_colnorm_kernel(const double* __restrict__ w, int len, double* __restrict__ sv) {
    __shared__ double lds[FR_THREADS];
    const double* __restrict__ col = w + (size_t)blockIdx.x * len;
    double s = 0.0;
    for (int e = threadIdx.x; e < len; e += FR_THREADS) s += col[e] * col[e];
    s = block_sum_fixed(s, lds);
    if (threadIdx.x == 0) sv[blockIdx.x] = sqrt(s);
}

int grid_for(size_t n) { return (int)std::min<size_t>((n + FR_THREADS - 1) / FR_THREADS, 4096); }

int launch_gram(const double* a, int n1, const double* b, int n2, int d, double* out, hipStream_t st) {
    const dim3 grid((n2 + GR_TILE - 1) / GR_TILE, (n1 + GR_TILE - 1) / GR_TILE);
    fr_gram_kernel<<<grid, FR_THREADS, 0, st>>>(a, n1, b, n2, d, out);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// Singular values of finite m [rows][cols], sorted descending, into sv (host).  Synchronises.
int jacobi_singular_values(const double* m, int rows, int cols, double tol, int max_sweeps, std::vector<double>& sv,
                           int* sweeps_out, hipStream_t st) {
    const bool transpose = cols <= rows;                 // the columns Jacobi works on: m's columns, or m's rows as they lie
    const int c = transpose ? cols : rows, len = transpose ? rows : cols;
    const int cpad = c + (c & 1);
    if (!(tol > 0.0)) tol = std::sqrt((double)len) * 0x1p-52;
    DevBuf w(st), aux(st);
    RLDM_HIP_CHECK(w.alloc((size_t)c * len * sizeof(double)));
    RLDM_HIP_CHECK(aux.alloc((size_t)c * sizeof(double) + sizeof(unsigned)));
    double* norms = aux.as<double>();
    unsigned* rotations = reinterpret_cast<unsigned*>(norms + c);
    if (transpose) {
        fr_transpose_kernel<<<grid_for((size_t)rows * cols), FR_THREADS, 0, st>>>(m, rows, cols, w.as<double>());
        RLDM_HIP_CHECK(hipGetLastError());
    } else {
        RLDM_HIP_CHECK(hipMemcpyAsync(w.p, m, (size_t)c * len * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    int sweeps = 0;
    bool converged = false;
    while (sweeps < max_sweeps) {
        RLDM_HIP_CHECK(hipMemsetAsync(rotations, 0, sizeof(unsigned), st));
        for (int step = 0; step < cpad - 1; ++step)
            fr_jacobi_step_kernel<<<cpad / 2, FR_THREADS, 0, st>>>(w.as<double>(), c, len, cpad, step, tol, rotations);
        RLDM_HIP_CHECK(hipGetLastError());
        unsigned applied = 0;
        RLDM_HIP_CHECK(hipMemcpyAsync(&applied, rotations, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        ++sweeps;
        if (applied == 0) { converged = true; break; }
    }
    if (sweeps_out) *sweeps_out = sweeps;
    if (!converged) {
        rldm::set_error("the Jacobi loop still rotated in sweep " + std::to_string(sweeps) + " (the cap) on a " +
                        std::to_string(len) + " x " + std::to_string(c) + " matrix; no value is returned");
        return RLDM_FRECHET_SWEEP_CAP;
    }
    fr_colnorm_kernel<<<c, FR_THREADS, 0, st>>>(w.as<double>(), len, norms);
    RLDM_HIP_CHECK(hipGetLastError());
    sv.resize(c);
    RLDM_HIP_CHECK(hipMemcpyAsync(sv.data(), norms, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    std::sort(sv.begin(), sv.end(), std::greater<double>());
    return 0;
}

}  // namespace

int rldm::check_finite_f64(std::initializer_list<std::pair<const double*, size_t>> arrays, hipStream_t st) {
    DevBuf flag(st);
    RLDM_HIP_CHECK(flag.alloc(sizeof(int)));
    RLDM_HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    for (const auto& arr : arrays) {
        if (!arr.first) continue;
        fr_finite_kernel<<<grid_for(arr.second), FR_THREADS, 0, st>>>(arr.first, arr.second, flag.as<int>());
        RLDM_HIP_CHECK(hipGetLastError());
    }
    int bad = 0;
    RLDM_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    if (bad) {
        rldm::set_error("the input holds NaN or inf; nothing was computed");
        return RLDM_FRECHET_NONFINITE;
    }
    return 0;
}

extern "C" {

int rldm_gram_f64(const double* a, int n1, const double* b, int n2, int d, double* out, void* stream) {
    RLDM_REQUIRE(a && b && out, "null argument");
    RLDM_REQUIRE(n1 > 0 && n2 > 0 && d > 0, "bad shape");
    RLDM_REQUIRE((long long)n1 * n2 < (1LL << 31), "matrix too large (n1 * n2 must stay below 2^31)");
    RLDM_REQUIRE(n1 <= GR_MAX_ROWS && n2 <= GR_MAX_ROWS, "too many rows (a grid dimension holds 65535 tiles of 64 rows)");
    return launch_gram(a, n1, b, n2, d, out, (hipStream_t)stream);
}

int rldm_singular_values_f64(const double* m, int rows, int cols, double tol, int max_sweeps, double* sv_out, int* sweeps_out,
                             void* stream) {
    RLDM_REQUIRE(m && sv_out, "null argument");
    RLDM_REQUIRE(rows > 0 && cols > 0, "bad shape");
    RLDM_REQUIRE((long long)rows * cols < (1LL << 31), "matrix too large (rows * cols must stay below 2^31)");
    RLDM_REQUIRE(max_sweeps >= 1, "max_sweeps must be at least 1");
    RLDM_REQUIRE(!(tol > 0.0) || std::isfinite(tol), "tol must be finite");
    hipStream_t st = (hipStream_t)stream;
    if (sweeps_out) *sweeps_out = 0;
    if (int rc = rldm::check_finite_f64({{m, (size_t)rows * cols}}, st)) return rc;
    std::vector<double> sv;
    if (int rc = jacobi_singular_values(m, rows, cols, tol, max_sweeps, sv, sweeps_out, st)) return rc;
    RLDM_HIP_CHECK(hipMemcpyAsync(sv_out, sv.data(), sv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int rldm_frechet_distance(const double* x, int n1, const double* y, int n2, int d, double* out5, void* stream) {
    RLDM_REQUIRE(x && y && out5, "null argument");
    RLDM_REQUIRE(n1 >= 2 && n2 >= 2 && d > 0, "each set needs at least 2 samples of d > 0 values");
    RLDM_REQUIRE((long long)n1 * d < (1LL << 31) && (long long)n2 * d < (1LL << 31) && (long long)n1 * n2 < (1LL << 31),
                 "set too large (n * d and n1 * n2 must stay below 2^31)");
    RLDM_REQUIRE(n1 <= GR_MAX_ROWS && n2 <= GR_MAX_ROWS, "too many samples (a grid dimension holds 65535 tiles of 64 rows)");
    hipStream_t st = (hipStream_t)stream;
    fr_last_sweeps = 0;
    if (int rc = rldm::check_finite_f64({{x, (size_t)n1 * d}, {y, (size_t)n2 * d}}, st)) return rc;

    // one allocation: A, B, M, mu1, mu2, rowsq1, rowsq2, totals
    const size_t na = (size_t)n1 * d, nb = (size_t)n2 * d, nm = (size_t)n1 * n2;
    DevBuf buf(st);
    RLDM_HIP_CHECK(buf.alloc((na + nb + nm + 2 * (size_t)d + n1 + n2 + 3) * sizeof(double)));
    double* A = buf.as<double>();
    double* B = A + na;
    double* M = B + nb;
    double* mu1 = M + nm;
    double* mu2 = mu1 + d;
    double* rowsq1 = mu2 + d;
    double* rowsq2 = rowsq1 + n1;
    double* totals = rowsq2 + n2;
    const int mean_grid = (d + FR_THREADS - 1) / FR_THREADS;
    fr_colmean_kernel<<<mean_grid, FR_THREADS, 0, st>>>(x, n1, d, mu1);
    fr_colmean_kernel<<<mean_grid, FR_THREADS, 0, st>>>(y, n2, d, mu2);
    fr_center_kernel<<<n1, FR_THREADS, 0, st>>>(x, mu1, d, A, rowsq1);
    fr_center_kernel<<<n2, FR_THREADS, 0, st>>>(y, mu2, d, B, rowsq2);
    fr_totals_kernel<<<1, FR_THREADS, 0, st>>>(rowsq1, n1, rowsq2, n2, mu1, mu2, d, totals);
    RLDM_HIP_CHECK(hipGetLastError());
    if (int rc = launch_gram(A, n1, B, n2, d, M, st)) return rc;

    std::vector<double> sv;
    int sweeps = 0;
    const int rc = jacobi_singular_values(M, n1, n2, 0.0, RLDM_FRECHET_MAX_SWEEPS, sv, &sweeps, st);
    fr_last_sweeps = sweeps;
    if (rc) return rc;
    double tot[3] = {0.0, 0.0, 0.0};
    RLDM_HIP_CHECK(hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    double nuclear = 0.0;
    for (double s : sv) nuclear += s;                    // descending, one add after the other
    const double tr1 = tot[0] / (double)(n1 - 1), tr2 = tot[1] / (double)(n2 - 1);
    const double trs = nuclear / std::sqrt((double)(n1 - 1) * (double)(n2 - 1));
    out5[0] = tot[2] + tr1 + tr2 - 2.0 * trs;
    out5[1] = tot[2];
    out5[2] = tr1;
    out5[3] = tr2;
    out5[4] = trs;
    return 0;
}

int rldm_frechet_last_sweeps(void) { return fr_last_sweeps; }

}  // extern "C"
