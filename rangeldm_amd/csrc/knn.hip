// knn.hip -- the K nearest neighbours of every point of a 3-D cloud in another cloud (or in its own), on gfx950, and the PCA
// surface normals that stand on them.  Point-to-plane Chamfer distance, normal consistency (pytorch3d's loss_normals) and the
// statistical outlier flag (rangeldm_amd/metrics.py) are read off these two.
//
//   knn_kernel<KT, R>    for every query point the K targets of its pair's other cloud that are smallest in the order
//                        (d^2 bits, target index), ascending in that order: exact, brute force
//   knn_normals_kernel   per point the covariance of the point and its neighbours in fp64, a cyclic Jacobi eigen-solve, the
//                        unit eigenvector of the smallest eigenvalue turned towards the sensor at the origin
//
// Numerics are nn_stream.h's (see its header): d^2 = ((dx*dx + dy*dy) + dz*dz) with dx = q - t, every operation one IEEE fp32
// rounding, so for K = 1 the row is rldm_nn_index's answer bit for bit, index included.
//
// Structure.  The tile, its staging and the grid plan are nn_stream.h's: a workgroup owns 256 x R query points in registers and
// streams the whole target cloud of its pair through an LDS tile that every lane reads in step.  The candidate loop is this
// file's own (scalar, and exactly the tile's n entries: a padding entry would be a candidate).  A query keeps its list as KT
// 64-bit keys (d^2 bits << 32) | index, ascending; non-negative floats order like their bit patterns.  The keys start as all ones, which
// sorts above +inf and is stored as the (+inf, -1) slot.  Targets arrive in ascending index order, so a candidate belongs in
// the list only if its d^2 bits are STRICTLY below the list's last: an equal one has a higher index than everything the list
// holds.  That one unsigned compare is all a target costs beyond its distance; a lane that passes it runs a fully unrolled
// compare-and-swap chain over the KT keys (keep the smaller, carry the larger; the carry that falls off the end is dropped).
// The keys are statically indexed throughout, so they live in VGPRs.
//
// Three tiers, 32 keys (64 VGPRs) per lane in each: KT = 8 with R = 4 queries per lane, KT = 16 with R = 2, KT = 32 with
// R = 1.  K rounds up to its tier and the store truncates.  A target cloud is never split over workgroups: one route, and a row
// depends on the two clouds of its pair alone.
#include "nn_stream.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d^2 is three products and two sums, each rounded

namespace {

constexpr int KN_KEYS = 32;                   // keys per lane in every tier: KT * R
constexpr int KN_MAX_K = 32;

typedef unsigned long long u64;
constexpr u64 KN_EMPTY = ~0ull;

// grid: one workgroup per (pair, block of 256 * R queries); wg_start[p] = first workgroup of pair p (num_pairs + 1 entries).
// self != 0: the target whose local index equals the query's is skipped (the clouds of a pair then have equal sizes).
// Four waves per SIMD: 128 VGPRs hold the 64 of the keys, the queries and the chain's carry without scratch.
template <int KT, int R>
__global__ __launch_bounds__(NN_THREADS, 4) void knn_kernel(const float* __restrict__ q, const int* __restrict__ qoff, int qstride,
                                                            const float* __restrict__ t, const int* __restrict__ toff,
                                                            int tstride, int num_pairs, const int* __restrict__ wg_start, int K,
                                                            int self, float* __restrict__ d2_out, int* __restrict__ idx_out) {
    static_assert(KT * R == KN_KEYS, "32 keys per lane");
    __shared__ float4 tile[NN_TILE];
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int p = segment_of(wg_start, num_pairs, wg);
    const int q0 = qoff[p], nq = qoff[p + 1] - q0, t0 = toff[p], nt = toff[p + 1] - t0;
    const int qb = wg - wg_start[p];

    float qx[R], qy[R], qz[R];
    int skip[R];                                         // the target index this query must not take (-1: none)
    u64 key[R][KT];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = min(qb * (NN_THREADS * R) + r * NN_THREADS + tid, nq - 1);     // past the end: a valid duplicate
        const float* pt = q + (size_t)(q0 + i) * qstride;
        qx[r] = pt[0]; qy[r] = pt[1]; qz[r] = pt[2];
        skip[r] = self ? i : -1;
#pragma unroll
        for (int s = 0; s < KT; ++s) key[r][s] = KN_EMPTY;
    }

    for (int base = 0; base < nt; base += NN_TILE) {
        const int n = min(NN_TILE, nt - base);
        stage_tile(tile, t, t0 + base, n, tstride, tid, false);     // no padding: nothing past n is read
        for (int j = 0; j < n; ++j) {                    // exactly n: a padding entry would be a candidate
            const float4 tp = tile[j];
            const int tj = base + j;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float dx = qx[r] - tp.x, dy = qy[r] - tp.y, dz = qz[r] - tp.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const unsigned bits = __float_as_uint(d2);
                if (bits < (unsigned)(key[r][KT - 1] >> 32) && tj != skip[r]) {
                    u64 carry = ((u64)bits << 32) | (unsigned)tj;
#pragma unroll
                    for (int s = 0; s < KT; ++s) {
                        const u64 k = key[r][s];
                        const bool below = carry < k;
                        key[r][s] = below ? carry : k;
                        carry = below ? k : carry;
                    }
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = qb * (NN_THREADS * R) + r * NN_THREADS + tid;
        if (i >= nq) continue;
        float* drow = d2_out + (size_t)(q0 + i) * K;
        int* irow = idx_out + (size_t)(q0 + i) * K;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            const u64 k = key[r][s];
            if (s < K) {
                drow[s] = k == KN_EMPTY ? INFINITY : __uint_as_float((unsigned)(k >> 32));
                irow[s] = k == KN_EMPTY ? -1 : (int)(unsigned)(k & 0xffffffffu);
            }
        }
    }
}

// one Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q); r is the third index.  app, aqq, apq are the plane's
// entries, arp, arq the third row's; v?p, v?q the two columns of the eigenvector matrix.  An off-diagonal entry that is exactly 0
// or below 2^-60 of the diagonal is left alone (the eigenvalues move by less than that).  t is computed in the form that
// cannot overflow into NaN: a huge theta gives t = 0.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                     double& v1p, double& v1q, double& v2p, double& v2q) {
    const bool rest = apq == 0.0 || fabs(apq) <= 0x1p-60 * (fabs(app) + fabs(aqq));      // then c = 1, s = 0: the identity, exactly
    const double theta = (aqq - app) / (2.0 * (rest ? 1.0 : apq));
    const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double tn = rest ? 0.0 : (theta < 0.0 ? -tt : tt);
    const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
    app -= tn * apq;
    aqq += tn * apq;
    apq = rest ? apq : 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double a = v0p, b = v0q;
    v0p = c * a - s * b; v0q = s * a + c * b;
    a = v1p; b = v1q;
    v1p = c * a - s * b; v1q = s * a + c * b;
    a = v2p; b = v2q;
    v2p = c * a - s * b; v2q = s * a + c * b;
}

constexpr int KN_SWEEPS = 8;                  // cyclic Jacobi on 3 x 3 converges quadratically: 8 sweeps are far past fp64

// one thread per point.  idx holds K local indices per point (rldm_knn with exclude_self); an entry outside the cloud (-1) is
// skipped.  The neighbourhood is the point itself, then its valid neighbours in slot order.
__global__ __launch_bounds__(256) void knn_normals_kernel(const float* __restrict__ pts, const int* __restrict__ off, int stride,
                                                          int num_clouds, const int* __restrict__ idx, int K,
                                                          double* __restrict__ normals, double* __restrict__ eig) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= off[num_clouds]) return;
    const int lo = segment_of(off, num_clouds, i);
    const int c0 = off[lo], n = off[lo + 1] - c0;
    const int* row = idx + (size_t)i * K;
    const float* self = pts + (size_t)i * stride;
    const double px = self[0], py = self[1], pz = self[2];
    double sx = px, sy = py, sz = pz;
    int m = 1;
    for (int s = 0; s < K; ++s) {
        const int j = row[s];
        if ((unsigned)j >= (unsigned)n) continue;
        const float* pt = pts + (size_t)(c0 + j) * stride;
        sx += (double)pt[0]; sy += (double)pt[1]; sz += (double)pt[2];
        ++m;
    }
    double* nout = normals + (size_t)i * 3;
    double* eout = eig + (size_t)i * 3;
    if (m < 3) {                                         // fewer than two valid neighbours: no plane
        nout[0] = nout[1] = nout[2] = 0.0;
        eout[0] = eout[1] = eout[2] = 0.0;
        return;
    }
    const double cx = sx / m, cy = sy / m, cz = sz / m;
    double a00, a01, a02, a11, a12, a22;
    {
        const double dx = px - cx, dy = py - cy, dz = pz - cz;
        a00 = dx * dx; a01 = dx * dy; a02 = dx * dz; a11 = dy * dy; a12 = dy * dz; a22 = dz * dz;
    }
    for (int s = 0; s < K; ++s) {
        const int j = row[s];
        if ((unsigned)j >= (unsigned)n) continue;
        const float* pt = pts + (size_t)(c0 + j) * stride;
        const double dx = (double)pt[0] - cx, dy = (double)pt[1] - cy, dz = (double)pt[2] - cz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
    }
    a00 /= m; a01 /= m; a02 /= m; a11 /= m; a12 /= m; a22 /= m;

    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < KN_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);       // (0, 1), third index 2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);       // (0, 2), third index 1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);       // (1, 2), third index 0
    }
    // ascending eigenvalues; the eigenvector of the smallest (the lowest column among equal ones)
    const bool first = a11 < a00;
    double e0 = first ? a11 : a00, e1 = first ? a00 : a11, e2 = a22;
    double nx = first ? v01 : v00, ny = first ? v11 : v10, nz = first ? v21 : v20;
    asm volatile("" : "+v"(nx), "+v"(ny), "+v"(nz));     // two selects, not one lookup in a table of columns (that table is scratch)
    const bool second = e2 < e0;
    nx = second ? v02 : nx; ny = second ? v12 : ny; nz = second ? v22 : nz;
    if (second) { const double e = e0; e0 = e2; e2 = e; }
    if (e2 < e1) { const double e = e1; e1 = e2; e2 = e; }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len; ny /= len; nz /= len;
    // towards the sensor at the origin: n . p <= 0; when that is 0, the first non-zero component is positive
    const double d = (nx * px + ny * py) + nz * pz;
    const double lead = nx != 0.0 ? nx : (ny != 0.0 ? ny : nz);
    if (d > 0.0 || (d == 0.0 && lead < 0.0)) { nx = -nx; ny = -ny; nz = -nz; }
    nout[0] = nx + 0.0; nout[1] = ny + 0.0; nout[2] = nz + 0.0;         // (+ 0.0: no negative zero leaves)
    eout[0] = e0; eout[1] = e1; eout[2] = e2;
}

template <int KT, int R>
void launch_knn(int grid, hipStream_t st, const float* q, const int* qoff, int qstride, const float* t, const int* toff, int tstride,
                int num_pairs, const int* wg_start, int K, int self, float* d2, int* idx) {
    knn_kernel<KT, R><<<grid, NN_THREADS, 0, st>>>(q, qoff, qstride, t, toff, tstride, num_pairs, wg_start, K, self, d2, idx);
}

}  // namespace

extern "C" {

int rldm_knn(const float* q, const int32_t* q_offsets, int q_stride, const float* t, const int32_t* t_offsets, int t_stride,
             int num_pairs, int K, int exclude_self, float* d2, int32_t* idx, void* stream) {
    RLDM_REQUIRE(q && q_offsets && t && t_offsets && d2 && idx, "null argument");
    RLDM_REQUIRE(num_pairs > 0 && q_stride >= 3 && t_stride >= 3, "bad shape");
    RLDM_REQUIRE(K >= 1 && K <= KN_MAX_K, "K must be in 1..32");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> qo(num_pairs + 1), to(num_pairs + 1);
    if (int rc = fetch_offsets(st, q_offsets, qo, t_offsets, to)) return rc;
    for (int p = 0; p < num_pairs; ++p)
        RLDM_REQUIRE(!exclude_self || qo[p + 1] - qo[p] == to[p + 1] - to[p], "exclude_self needs clouds of equal sizes");
    const int R = K <= 8 ? 4 : (K <= 16 ? 2 : 1);
    PairGrid wgs(st);                                    // a target cloud is never split
    if (int rc = wgs.plan(qo, to, NN_THREADS * R, 0)) return rc;
    if (int rc = wgs.upload()) return rc;
    const int32_t* dstarts = wgs.dev.as<int32_t>();
    const int grid = wgs.host[num_pairs], self = exclude_self ? 1 : 0;
    if (R == 4) launch_knn<8, 4>(grid, st, q, q_offsets, q_stride, t, t_offsets, t_stride, num_pairs, dstarts, K, self, d2, idx);
    else if (R == 2) launch_knn<16, 2>(grid, st, q, q_offsets, q_stride, t, t_offsets, t_stride, num_pairs, dstarts, K, self, d2, idx);
    else launch_knn<32, 1>(grid, st, q, q_offsets, q_stride, t, t_offsets, t_stride, num_pairs, dstarts, K, self, d2, idx);
    RLDM_HIP_CHECK(hipGetLastError());
    return wgs.finish();
}

int rldm_knn_normals(const float* pts, const int32_t* offsets, int stride, int num_clouds, const int32_t* idx, int K,
                     double* normals, double* eigenvalues, void* stream) {
    RLDM_REQUIRE(pts && offsets && idx && normals && eigenvalues, "null argument");
    RLDM_REQUIRE(num_clouds > 0 && stride >= 3, "bad shape");
    RLDM_REQUIRE(K >= 1 && K <= KN_MAX_K, "K must be in 1..32");
    hipStream_t st = (hipStream_t)stream;
    int32_t total = 0;
    RLDM_HIP_CHECK(hipMemcpyAsync(&total, offsets + num_clouds, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    RLDM_REQUIRE(total > 0 && (long long)total + 255 < (1LL << 31), "bad offsets");
    knn_normals_kernel<<<(total + 255) / 256, 256, 0, st>>>(pts, offsets, stride, num_clouds, idx, K, normals, eigenvalues);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
