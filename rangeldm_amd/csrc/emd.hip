// emd.hip -- Earth Mover's Distance between equal-size point clouds on gfx950: an epsilon-scaling forward AUCTION
// (Bertsekas), exact in the sense that it returns an assignment and dual prices that certify its distance from the optimum
// (DESIGN.md 3.1).  Every arithmetic step is one correctly rounded fp32 operation, so a sequential CPU restatement
// (tests/test_emd_host.py: auction_host) reproduces assignment, prices, bid count and value bit for bit.
//
//   emd_auction_kernel<K>   one pair of clouds per wave (a workgroup IS one wave: no barrier in the bidding loop, no atomics
//                           on the result); lane l owns the objects j = l + 64 k, k < K, of Y and keeps their xyz in VGPRs
//
// Cost.      c[i][j] = sqrtf((dx*dx + dy*dy) + dz*dz), dx = x_i - y_j: no FMA contraction (the pragma below and
//            -ffp-contract=off in the Makefile), IEEE sqrt (-fhip-fp32-correctly-rounded-divide-sqrt in the Makefile), fp32
//            denormals kept (-fno-gpu-flush-denormals-to-zero).
// Auction.   Points of X bid for points of Y.  Unassigned bidders wait in a FIFO that starts as 0 .. N-1.  The head i takes
//            w[j] = c[i][j] + p[j] over all objects, the smallest w1 at j1 (LOWEST j on ties) and the second smallest w2
//            (over j != j1; w2 = w1 for N = 1), sets p[j1] = (p[j1] + (w2 - w1)) + eps, takes j1 and sends j1's previous
//            owner to the tail.  (With v = -w this is the textbook p += (v1 - v2) + eps: fp32 negation is exact, so
//            v1 - v2 == w2 - w1 bit for bit.)  A phase ends when the FIFO is empty.
// Scaling.   e_0 = 0.25f * ext, ext = the largest fp32 side (hi - lo) of the joint bounding box of the two clouds; phase
//            k runs with max(e_k, eps) and e_{k+1} = e_k * 0.25f; the phase whose e_k <= eps is the last.  Prices carry
//            over, assignments are reset.
// Value.     the fp64 sum of c[i][a(i)], i ascending, one add after the other, divided once by N.
// Bid cap.   a pair that has made 1024 N bids with bidders still waiting stops; the call reports it (no partial value).
//
// Wave-uniform bookkeeping.  After the butterfly every lane holds the same (w1, j1, w2); every lane then performs the same
// LDS writes (price, owner, FIFO) with the same value, so each lane only ever reads back what it wrote itself: the bidding
// loop needs no barrier.  __syncthreads() (one wave: cheap) separates the few places where lanes write different slots.
//
// Preconditions: both clouds of a pair hold the same N <= 2048 points (checked on the host from the offsets); coordinates
// are finite -- NaN or inf inputs give unspecified results, but the bid cap still ends every pair.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <climits>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) every cost and price step is a single IEEE op

namespace {

constexpr int EMD_WAVE = 64;
constexpr int EMD_BIDS_PER_POINT = 1024;     // the bid cap, per point
constexpr unsigned short EMD_NONE = 0xffff;

__device__ __forceinline__ float emd_cost(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
}

// grid: one single-wave workgroup per entry of the (nx, ny) layout (mode RECT / SYMMETRIC) or per diagonal entry (DIAGONAL).
// dynamic LDS: 64 * K prices (fp32), 64 * K owners and a ring of 64 * K (uint16 each): 512 * K bytes, 16 KiB at K = 32.
template <int K>
__global__ __launch_bounds__(EMD_WAVE) void emd_auction_kernel(const float* __restrict__ x, const int* __restrict__ xoff,
                                                               int xs, const float* __restrict__ y,
                                                               const int* __restrict__ yoff, int ys, int ny, int mode,
                                                               float eps, double* __restrict__ emd_out,
                                                               int* __restrict__ assign_out, float* __restrict__ price_out,
                                                               int* __restrict__ bids_out, int* __restrict__ flag) {
    extern __shared__ float emd_lds[];
    constexpr int CAP = EMD_WAVE * K;
    float* price = emd_lds;
    unsigned short* owner = reinterpret_cast<unsigned short*>(price + CAP);
    unsigned short* fifo = owner + CAP;
    const int lane = threadIdx.x;
    int pi, pj;
    if (mode == RLDM_EMD_DIAGONAL) {
        pi = pj = blockIdx.x;
    } else {
        pi = blockIdx.x / ny;
        pj = blockIdx.x - pi * ny;
        if (mode == RLDM_EMD_SYMMETRIC && pj <= pi) return;
    }
    const int N = xoff[pi + 1] - xoff[pi];
    const float* __restrict__ X = x + (size_t)xoff[pi] * xs;
    const float* __restrict__ Y = y + (size_t)yoff[pj] * ys;

    // this lane's objects (pad slots at +inf: their cost is +inf and never wins) and the joint bounding box
    float ox[K], oy[K], oz[K];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = lane + EMD_WAVE * k;
        ox[k] = oy[k] = oz[k] = INFINITY;
        if (j < N) {
            const float* pt = Y + (size_t)j * ys;
            ox[k] = pt[0]; oy[k] = pt[1]; oz[k] = pt[2];
            lo[0] = fminf(lo[0], ox[k]); lo[1] = fminf(lo[1], oy[k]); lo[2] = fminf(lo[2], oz[k]);
            hi[0] = fmaxf(hi[0], ox[k]); hi[1] = fmaxf(hi[1], oy[k]); hi[2] = fmaxf(hi[2], oz[k]);
        }
        price[j] = 0.f;
    }
    for (int i = lane; i < N; i += EMD_WAVE) {
        const float* pt = X + (size_t)i * xs;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], pt[d]);
            hi[d] = fmaxf(hi[d], pt[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o; o >>= 1) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], o));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o));
        }
    }
    float e = 0.25f * fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);

    const int cap = EMD_BIDS_PER_POINT * N;
    int bids = 0;
    bool capped = false;
    for (;;) {
        const float ek = e > eps ? e : eps;
        __syncthreads();                                 // the previous phase's reads are done
#pragma unroll
        for (int k = 0; k < K; ++k) {
            owner[lane + EMD_WAVE * k] = EMD_NONE;
            fifo[lane + EMD_WAVE * k] = (unsigned short)(lane + EMD_WAVE * k);
        }
        __syncthreads();
        int head = 0, tail = N == CAP ? 0 : N, count = N;
        int cur = 0;
        float cx = X[0], cy = X[1], cz = X[2];
        while (count > 0) {
            if (bids >= cap) { capped = true; break; }
            head = head + 1 == CAP ? 0 : head + 1;       // pop `cur`
            --count;
            // the next head, if it is already known, so that its coordinates arrive under this bid's arithmetic
            int nxt = -1;
            float nx = 0.f, nyy = 0.f, nz = 0.f;
            if (count > 0) {
                nxt = __builtin_amdgcn_readfirstlane((int)fifo[head]);
                const float* pt = X + (size_t)nxt * xs;
                nx = pt[0]; nyy = pt[1]; nz = pt[2];
            }
            // this lane's two smallest w, ascending j (a strict < keeps the lowest j)
            float w1 = INFINITY, w2 = INFINITY;
            int k1 = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float w = emd_cost(cx, cy, cz, ox[k], oy[k], oz[k]) + price[lane + EMD_WAVE * k];
                w2 = fminf(w2, fmaxf(w, w1));
                k1 = w < w1 ? k : k1;
                w1 = fminf(w1, w);
            }
            int j1 = lane + EMD_WAVE * k1;
            // butterfly: smaller w, else smaller j, wins; the loser's best is a candidate for second place
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                const float q1 = __shfl_xor(w1, o), q2 = __shfl_xor(w2, o);
                const int qj = __shfl_xor(j1, o);
                const bool other = q1 < w1 || (q1 == w1 && qj < j1);
                w2 = other ? fminf(q2, w1) : fminf(w2, q1);
                w1 = other ? q1 : w1;
                j1 = other ? qj : j1;
            }
            if (N == 1) w2 = w1;
            j1 = __builtin_amdgcn_readfirstlane(j1);
            price[j1] = (price[j1] + (w2 - w1)) + ek;
            const int prev = __builtin_amdgcn_readfirstlane((int)owner[j1]);
            owner[j1] = (unsigned short)cur;
            ++bids;
            if (prev != EMD_NONE) {
                fifo[tail] = (unsigned short)prev;
                tail = tail + 1 == CAP ? 0 : tail + 1;
                ++count;
                if (nxt < 0) {                           // the queue was empty: the displaced bidder is next
                    nxt = prev;
                    const float* pt = X + (size_t)nxt * xs;
                    nx = pt[0]; nyy = pt[1]; nz = pt[2];
                }
            }
            cur = nxt;
            cx = nx; cy = nyy; cz = nz;
        }
        if (capped || !(e > eps)) break;
        e = e * 0.25f;
    }

    const size_t entry = (size_t)pi * ny + pj, mirror = (size_t)pj * ny + pi;
    if (capped) {                                        // never a partial value: NaN, and the call fails naming the pair
        if (lane == 0) {
            atomicMin(flag, (int)blockIdx.x);
            emd_out[entry] = NAN;
            if (mode == RLDM_EMD_SYMMETRIC) emd_out[mirror] = NAN;
        }
        return;
    }
    // every object is owned now.  a(i) goes into the (empty) ring, then c[i][a(i)] replaces this lane's own price slots
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = lane + EMD_WAVE * k;
        if (j < N && owner[j] < N) fifo[owner[j]] = (unsigned short)j;      // (owned by construction; the test keeps the index in bounds)
    }
    __syncthreads();
    const size_t base = entry * (size_t)N;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = lane + EMD_WAVE * k;
        if (i < N) {
            const int a = min((int)fifo[i], N - 1);
            if (assign_out) assign_out[base + i] = a;
            if (price_out) price_out[base + i] = price[i];
            const float* p = X + (size_t)i * xs;
            const float* q = Y + (size_t)a * ys;
            price[i] = emd_cost(p[0], p[1], p[2], q[0], q[1], q[2]);
        }
    }
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += (double)price[i];   // i ascending, one add after the other (every lane the same)
    if (lane == 0) {
        const double v = s / (double)N;
        emd_out[entry] = v;
        if (bids_out) bids_out[entry] = bids;
        if (mode == RLDM_EMD_SYMMETRIC) {
            emd_out[mirror] = v;
            if (bids_out) bids_out[mirror] = bids;
        }
    }
}

template <int K>
hipError_t launch_emd(int grid, hipStream_t st, const float* x, const int* xoff, int xs, const float* y, const int* yoff, int ys,
                      int ny, int mode, float eps, double* emd_out, int* assign_out, float* price_out, int* bids_out, int* flag) {
    const size_t lds = (size_t)EMD_WAVE * K * (sizeof(float) + 2 * sizeof(unsigned short));     // at most 16 KiB
    emd_auction_kernel<K><<<grid, EMD_WAVE, lds, st>>>(x, xoff, xs, y, yoff, ys, ny, mode, eps, emd_out, assign_out, price_out,
                                                       bids_out, flag);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int rldm_emd_matrix(const float* x, const int32_t* x_offsets, int x_stride, int nx, const float* y, const int32_t* y_offsets,
                    int y_stride, int ny, int symmetric, float eps, double* emd_out, int32_t* assign_out, float* price_out,
                    int32_t* bids_out, void* stream) {
    RLDM_REQUIRE(x && x_offsets && y && y_offsets && emd_out, "null argument");
    RLDM_REQUIRE(nx > 0 && ny > 0 && x_stride >= 3 && y_stride >= 3, "bad shape");
    RLDM_REQUIRE(symmetric == RLDM_EMD_RECT || symmetric == RLDM_EMD_SYMMETRIC || symmetric == RLDM_EMD_DIAGONAL,
                 "symmetric must be 0 (rectangular), 1 (symmetric) or 2 (diagonal only)");
    RLDM_REQUIRE(symmetric != RLDM_EMD_SYMMETRIC || (x == y && x_offsets == y_offsets && x_stride == y_stride && nx == ny),
                 "symmetric: y must be x (the same buffers)");
    RLDM_REQUIRE(symmetric != RLDM_EMD_DIAGONAL || nx == ny, "diagonal: nx must equal ny");
    RLDM_REQUIRE((long long)nx * ny < (1LL << 31), "matrix too large (nx * ny must stay below 2^31)");
    RLDM_REQUIRE(eps > 0.f && std::isfinite(eps), "eps must be positive and finite");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> xo(nx + 1), yo(ny + 1);
    if (int rc = fetch_offsets(st, x_offsets, xo, y_offsets, yo)) return rc;
    const int N = xo[1] - xo[0];
    RLDM_REQUIRE(N >= 1 && N <= RLDM_EMD_MAX_POINTS, "clouds must hold 1 to 2048 points");
    for (int c = 0; c < nx; ++c) RLDM_REQUIRE(xo[c + 1] - xo[c] == N, "EMD is a one-to-one matching: every cloud must hold the same number of points");
    for (int c = 0; c < ny; ++c) RLDM_REQUIRE(yo[c + 1] - yo[c] == N, "EMD is a one-to-one matching: every cloud must hold the same number of points");

    DevBuf fbuf(st);
    RLDM_HIP_CHECK(fbuf.alloc(sizeof(int)));
    int* flag = fbuf.as<int>();
    RLDM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flag), INT_MAX, 1, st));
    if (symmetric == RLDM_EMD_SYMMETRIC) {               // the diagonal; every other entry is written by its pair
        RLDM_HIP_CHECK(hipMemsetAsync(emd_out, 0, (size_t)nx * ny * sizeof(double), st));
        if (bids_out) RLDM_HIP_CHECK(hipMemsetAsync(bids_out, 0, (size_t)nx * ny * sizeof(int32_t), st));
    }
    const int grid = symmetric == RLDM_EMD_DIAGONAL ? nx : nx * ny;
    const int k = (N + EMD_WAVE - 1) / EMD_WAVE;         // objects per lane; the instances below pad it up
    hipError_t err;
#define EMD_LAUNCH(K) launch_emd<K>(grid, st, x, x_offsets, x_stride, y, y_offsets, y_stride, ny, symmetric, eps, emd_out, \
                                    assign_out, price_out, bids_out, flag)
    if (k <= 1) err = EMD_LAUNCH(1);
    else if (k <= 2) err = EMD_LAUNCH(2);
    else if (k <= 4) err = EMD_LAUNCH(4);
    else if (k <= 8) err = EMD_LAUNCH(8);
    else if (k <= 16) err = EMD_LAUNCH(16);
    else if (k <= 24) err = EMD_LAUNCH(24);
    else err = EMD_LAUNCH(32);
#undef EMD_LAUNCH
    RLDM_HIP_CHECK(err);
    int flagged = INT_MAX;
    RLDM_HIP_CHECK(hipMemcpyAsync(&flagged, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    if (flagged != INT_MAX) {
        const int i = symmetric == RLDM_EMD_DIAGONAL ? flagged : flagged / ny;
        const int j = symmetric == RLDM_EMD_DIAGONAL ? flagged : flagged - i * ny;
        rldm::set_error("pair (" + std::to_string(i) + ", " + std::to_string(j) + ") reached the bid cap of " +
                        std::to_string(EMD_BIDS_PER_POINT) + " x " + std::to_string(N) + " bids; no value is returned");
        return RLDM_EMD_BID_CAP;
    }
    return 0;
}

}  // extern "C"
