// fps.hip -- farthest point sampling on gfx950: the sub-sampling step of the point-cloud generation metrics (PointFlow's
// MMD / COV / 1-NNA protocol), k strictly sequential rounds per cloud, each an update of the min-distance array and an
// arg-max over the whole cloud.  Every arithmetic step is one correctly rounded fp32 operation, so a sequential numpy
// restatement (tests/test_fps_host.py: fps_host) reproduces the selected indices exactly.
//
//   fps_kernel    one workgroup of FPS_BLOCK = 1024 lanes per cloud; no workgroup ever waits on another, no atomics
//
// Rounds.    mind[i] = +inf; sel = start.  Round t emits sel, then
//              d = ((dx*dx + dy*dy) + dz*dz), dx = x[i] - x[sel]      (chamfer.hip's expression and association; no FMA
//                                                                      contraction: the pragma below and the Makefile)
//              mind[i] = min(mind[i], d);  mind[sel] = -inf;  sel = argmax mind, the LOWEST index on ties.
//            The -inf sentinel is below every distance, so an index is never selected twice: the k indices are distinct even
//            on a cloud of duplicates (k <= P leaves an unselected point, at mind >= 0, in every round).  The kernel plants
//            the sentinel before the min instead of after it -- min(-inf, d) = -inf, the same array.
// Tiers.     Point i of a cloud belongs to lane i mod 1024.  The first FPS_RESIDENT = 64 x 1024 points keep mind in
//            VGPRs (64 per lane: with 16 waves per workgroup, 4 per SIMD, a lane has 128); the points past them keep it
//            in a global workspace that the owning lane alone reads and writes (it stays in L2 between rounds).  A cloud
//            of at most 65 536 points -- a generated range image -- never touches the workspace.
// Coordinates.  The first 12 x 1024 points' xyz are staged in LDS once (144 KiB; a lane reads back only its own entries,
//            so no barrier); the others are re-read every round (a cloud is at most 1.5 MB at 12-16 B per point: it is
//            served from L2 / the Infinity Cache / HBM), one group of four points per lane requested while the group before
//            it is computed.  With every CU on a 65 536-point cloud the re-reads are what a round costs; staging measured
//            faster than re-reading everything.  Offsets into a cloud are 32-bit: P * stride * 4 < 2^31.
// Arg-max.   Three levels, each carrying (value, index) with the lowest-index rule.  Per lane: points in ascending index,
//            a strict > keeps the first.  Then one 64-bit key per lane: the high word orders mind (-inf -> 0, a
//            non-negative float -> its bit pattern + 1: non-negative floats order like their bits), the low word is ~index,
//            so the unsigned maximum is the largest mind at the lowest index.  Per wave a shuffle butterfly; across the 16
//            waves one LDS slot each, double-buffered by round parity: ONE barrier per round (a wave can only overwrite a
//            buffer two rounds later, after every wave has passed the barrier in between).
//
// Preconditions (checked on the host from the offsets): 1 <= k <= P <= RLDM_FPS_MAX_POINTS, 0 <= start < P.  Coordinates
// are finite (the Python layer refuses others): min / arg-max over NaN is not a defined order.  Even so no index leaves
// [0, P): a NaN never passes the strict > that tracks a lane's best, every coordinate offset is clamped to the cloud's last
// point, and the winner is clamped to [0, P) before it is used or written.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <string>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) d is three subtractions, three products, two sums

namespace {

constexpr int FPS_BLOCK = RLDM_FPS_BLOCK;
constexpr int FPS_WAVES = FPS_BLOCK / 64;
constexpr int FPS_R = 64;                     // resident points per lane
constexpr int FPS_G = 4;                      // points per lane in a group: one group computed, the next in flight
constexpr int FPS_RESIDENT = FPS_BLOCK * FPS_R;
constexpr int FPS_LDS_SLOTS = 12;             // slots per lane whose coordinates are staged in LDS: 12 x 1024 x 12 B = 144 KiB
constexpr size_t FPS_LDS_BYTES = (size_t)3 * FPS_LDS_SLOTS * FPS_BLOCK * sizeof(float);
static_assert(FPS_LDS_SLOTS % FPS_G == 0 && FPS_LDS_SLOTS <= FPS_R, "whole groups are staged");
static_assert(FPS_RESIDENT == RLDM_FPS_RESIDENT_POINTS, "the header states the resident tier");
static_assert(FPS_LDS_SLOTS * FPS_BLOCK == RLDM_FPS_STAGED_POINTS, "the header states the staged (LDS) tier");
static_assert(FPS_G * FPS_BLOCK == RLDM_FPS_GROUP_POINTS, "the header states the group");
static_assert(FPS_WAVES == 16, "the workgroup level reads one slot per lane & 15");

typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

__device__ __forceinline__ u64 fps_key(float m, int i) {
    const unsigned hi = m < 0.f ? 0u : __float_as_uint(m) + 1u;          // mind is -inf or >= +0
    return ((u64)hi << 32) | (unsigned)~i;
}

// v_min_f32 as it is: fminf would first re-quiet the loop-carried operand (one more instruction per point), and neither
// operand is ever a signalling NaN here
__device__ __forceinline__ float min_f32(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// row `row` (of FPS_BLOCK floats) of this lane's LDS column: three bases 64 KiB apart, so that every access is a base plus an
// immediate offset (a DS offset has 16 bits) and no per-row address sits in a register
__device__ __forceinline__ float& lds_at(float* const (&base)[3], int row) { return base[row / 16][(row % 16) * RLDM_FPS_BLOCK]; }

__device__ __forceinline__ u64 key_max(u64 a, u64 b) { return a > b ? a : b; }

// grid: one workgroup per cloud.  ws (fp32, indexed like the packed points) is only touched by clouds above FPS_RESIDENT.
__global__ __launch_bounds__(FPS_BLOCK) void fps_kernel(const float* __restrict__ x, const int* __restrict__ off, int stride,
                                                        int k, const int* __restrict__ start, float* __restrict__ ws,
                                                        int* __restrict__ out) {
    __shared__ u64 slot[2][FPS_WAVES];
    extern __shared__ float fps_lds[];                                   // [FPS_LDS_SLOTS][3][FPS_BLOCK]: slot, x / y / z, lane
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = off[c], P = off[c + 1] - q0;
    const char* __restrict__ X = reinterpret_cast<const char*>(x + (size_t)q0 * stride);
    const unsigned step = (unsigned)stride * 4u;                         // bytes per point
    const unsigned off_last = (unsigned)(P - 1) * step;                  // offsets are clamped to the last point, never past it
    const unsigned off_tid = (unsigned)tid * step, blk_step = (unsigned)FPS_BLOCK * step;
    float* __restrict__ W = ws + q0;
    int* __restrict__ o = out + (size_t)c * k;

    float mind[FPS_R];                                                   // slot j is point tid + j * FPS_BLOCK; past P: -inf
#pragma unroll
    for (int j = 0; j < FPS_R; ++j) mind[j] = tid + j * FPS_BLOCK < P ? INFINITY : -INFINITY;
    for (int i = FPS_RESIDENT + tid; i < P; i += FPS_BLOCK) W[i] = INFINITY;
    // the first FPS_LDS_SLOTS slots' coordinates go to LDS once.  A lane reads back only what it wrote itself: no barrier
    float* lb[3] = {fps_lds + tid, fps_lds + tid + 16 * FPS_BLOCK, fps_lds + tid + 32 * FPS_BLOCK};
#pragma unroll
    for (int j = 0; j < FPS_LDS_SLOTS; ++j) {
        if (j * FPS_BLOCK < P) {                                         // (uniform; slots past it are never read)
            const float* pt = reinterpret_cast<const float*>(X + min(off_tid + (unsigned)j * blk_step, off_last));
            lds_at(lb, j * 3) = pt[0]; lds_at(lb, j * 3 + 1) = pt[1]; lds_at(lb, j * 3 + 2) = pt[2];
        }
    }

    int sel = start ? start[c] : 0;
    sel = __builtin_amdgcn_readfirstlane(min(max(sel, 0), P - 1));
    for (int t = 0;; ++t) {
        if (tid == 0) o[t] = sel;
        if (t == k - 1) break;                                           // (uniform) the last index needs no update
        const float* sp = reinterpret_cast<const float*>(X + (size_t)sel * step);
        const float sx = sp[0], sy = sp[1], sz = sp[2];
        const f2 cxy = f2{sx, sy};

        // the sentinel goes to slot sel / 1024 of lane sel % 1024; the slot is uniform over the workgroup
        const int jsel = sel / FPS_BLOCK;
        const bool own = (sel & (FPS_BLOCK - 1)) == tid;
        float best = -INFINITY;
        int bj = 0;
        unsigned at = off_tid + (unsigned)FPS_LDS_SLOTS * blk_step;      // this lane's byte offset, slot by slot
        // the coordinates of group g: from LDS for the staged slots, else from memory (clamped to the last point)
        auto load_group = [&](int g, float (&v)[FPS_G][3]) {
#pragma unroll
            for (int u = 0; u < FPS_G; ++u) {
                if (g * FPS_G < FPS_LDS_SLOTS) {
                    v[u][0] = lds_at(lb, (g * FPS_G + u) * 3); v[u][1] = lds_at(lb, (g * FPS_G + u) * 3 + 1);
                    v[u][2] = lds_at(lb, (g * FPS_G + u) * 3 + 2);
                } else {
                    const float* pt = reinterpret_cast<const float*>(X + min(at, off_last));
                    at += blk_step;
                    v[u][0] = pt[0]; v[u][1] = pt[1]; v[u][2] = pt[2];
                }
            }
        };
        float v[2][FPS_G][3];                                            // group g + 1 arrives under group g's arithmetic
        load_group(0, v[0]);
#pragma unroll
        for (int g = 0; g < FPS_R / FPS_G; ++g) {
            if (g * FPS_G * FPS_BLOCK < P) {                             // (uniform) a group past the cloud holds only -inf
                if (g + 1 < FPS_R / FPS_G && (g + 1) * FPS_G * FPS_BLOCK < P) load_group(g + 1, v[(g + 1) & 1]);
                if (jsel / FPS_G == g) {                                 // (uniform)
#pragma unroll
                    for (int u = 0; u < FPS_G; ++u)
                        if (jsel == g * FPS_G + u) mind[g * FPS_G + u] = own ? -INFINITY : mind[g * FPS_G + u];
                }
#pragma unroll
                for (int u = 0; u < FPS_G; ++u) {
                    const int j = g * FPS_G + u;
                    const f2 dxy = f2{v[g & 1][u][0], v[g & 1][u][1]} - cxy;       // x and y of one point as a packed pair
                    const float dz = v[g & 1][u][2] - sz;
                    const f2 sq = dxy * dxy;
                    const float m = min_f32(mind[j], (sq.x + sq.y) + dz * dz);
                    mind[j] = m;
                    if (m > best) { best = m; bj = j; }                  // ascending index: a strict > keeps the lowest
                }
            }
        }
        int bi = tid + bj * FPS_BLOCK;
        // second tier: this lane's points past the resident ones, mind in the workspace, FPS_G points in flight
        for (int base = FPS_RESIDENT; base < P; base += FPS_G * FPS_BLOCK) {           // (uniform)
            float v[FPS_G][3], m[FPS_G];
#pragma unroll
            for (int u = 0; u < FPS_G; ++u) {
                const int i = base + u * FPS_BLOCK + tid, ic = min(i, P - 1);
                const float* pt = reinterpret_cast<const float*>(X + (unsigned)ic * step);
                v[u][0] = pt[0]; v[u][1] = pt[1]; v[u][2] = pt[2];
                m[u] = i < P && i != sel ? W[ic] : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < FPS_G; ++u) {
                const int i = base + u * FPS_BLOCK + tid;
                const float dx = v[u][0] - sx, dy = v[u][1] - sy, dz = v[u][2] - sz;
                const float r = min_f32(m[u], (dx * dx + dy * dy) + dz * dz);
                if (i < P) W[i] = r;
                if (r > best) { best = r; bi = i; }                      // (past P: -inf, never above best)
            }
        }

        u64 key = fps_key(best, bi);
#pragma unroll
        for (int s = 32; s; s >>= 1) key = key_max(key, __shfl_xor(key, s));
        if (lane == 0) slot[t & 1][wave] = key;
        __syncthreads();
        key = slot[t & 1][lane & (FPS_WAVES - 1)];
#pragma unroll
        for (int s = FPS_WAVES / 2; s; s >>= 1) key = key_max(key, __shfl_xor(key, s));
        sel = __builtin_amdgcn_readfirstlane((int)~(unsigned)key);
        sel = min(max(sel, 0), P - 1);                                   // (a no-op on finite input)
    }
}

}  // namespace

extern "C" {

int rldm_farthest_point_sample(const float* x, const int32_t* offsets, int stride, int num_clouds, int k, const int32_t* start,
                               int32_t* idx_out, void* stream) {
    RLDM_REQUIRE(x && offsets && idx_out, "null argument");
    RLDM_REQUIRE(num_clouds > 0 && stride >= 3 && k >= 1, "bad shape");
    RLDM_REQUIRE((long long)num_clouds * k < (1LL << 31), "too many indices (num_clouds * k must stay below 2^31)");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> off(num_clouds + 1), first(start ? num_clouds : 0);
    if (start) RLDM_HIP_CHECK(hipMemcpyAsync(first.data(), start, first.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (int rc = fetch_offsets(st, offsets, off)) return rc;      // its synchronise covers `first` too
    int largest = 0;
    for (int c = 0; c < num_clouds; ++c) {
        const long long P = (long long)off[c + 1] - off[c];
        const std::string who = "cloud " + std::to_string(c) + ": ";
        RLDM_REQUIRE(P <= RLDM_FPS_MAX_POINTS, who + "more than RLDM_FPS_MAX_POINTS (1048576) points");
        RLDM_REQUIRE(P * stride * 4 < (1LL << 31), who + "points x stride too large (byte offsets into a cloud are 32-bit)");
        RLDM_REQUIRE(k <= P, who + "k exceeds the number of points");
        RLDM_REQUIRE(!start || (first[c] >= 0 && first[c] < P), who + "start must be an index of the cloud");
        largest = std::max(largest, (int)P);
    }
    static rldm::DynLdsLimit lds_limit;
    RLDM_HIP_CHECK(lds_limit.ensure(reinterpret_cast<const void*>(&fps_kernel), FPS_LDS_BYTES));
    {   // the workspace goes back to the pool before the wait below, not after it: measured 1 % on a 131 072-point cloud
        DevBuf ws(st);                                   // the second tier's min-distances, one fp32 per packed point
        if (largest > FPS_RESIDENT) RLDM_HIP_CHECK(ws.alloc((size_t)off[num_clouds] * sizeof(float)));
        fps_kernel<<<num_clouds, FPS_BLOCK, FPS_LDS_BYTES, st>>>(x, offsets, stride, k, start, ws.as<float>(), idx_out);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    RLDM_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
