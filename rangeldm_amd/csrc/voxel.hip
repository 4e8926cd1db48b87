// voxel.hip -- voxel-occupancy counts of a reconstructed cloud against its target on gfx950: the integers behind the
// occupancy IoU / precision / recall / F1 that the LiDAR up-sampling and completion tables list next to MAE and CD.
//
//   voxel_insert_kernel   every point of a chunk of pairs into its pair's hash set of occupied voxels
//   voxel_count_kernel    per pair the number of voxels the result holds (a), the target holds (b), and both hold (c)
//
// Definition.  v = (float)voxel.  q(c) = floorf(c / v): ONE correctly rounded fp32 division (eval_common.h's f_div; the
// Makefile gives this file -fhip-fp32-correctly-rounded-divide-sqrt and -fno-gpu-flush-denormals-to-zero, so
// floorf(-1e-40f / 0.1f) is -1 as in numpy), then floorf.  A point's voxel is (q(x), q(y), q(z)).  A point is in range when
// -2^20 <= q < 2^20 on every axis -- NaN and inf coordinates fail that comparison, so the one test covers them.  A call that
// holds a point out of range reports nothing (RLDM_VOXEL_RANGE).  a, b, c are counts of distinct keys: they do not depend on
// the order of the points, on the other pairs of the call, or on the chunking below.
//
// Table.  One 64-bit word per slot: bit 63 set (a claimed slot is never 0, the cleared state) and the three 21-bit biased
// indices q + 2^20 in bits 0-20, 21-41, 42-62.  Three 21-bit indices leave one bit, not two, so the two membership bits of a
// slot (1: the result holds the voxel, 2: the target does) live in a bitmap beside the table, two bits per slot, sixteen slots
// per 32-bit word.  A pair's table has VOX_MIN_SLOTS or the power of two >= 2 (n + m) slots, whichever is larger: at most
// half of it is ever claimed, so a probe always ends at an empty slot or at its own key.
//
// Only atomics touch the table while it is filled.  A point hashes its key, then walks linearly: atomicCAS(slot, 0, key)
// returns 0 (claimed now) or the key (claimed before, by either side) -> atomicOr of the side's bit into the bitmap, done;
// any other value -> next slot.  The value the CAS returns IS the probe: a plain load could be served from the CU's L1 or
// the XCD's L2, neither of which sees another CU's atomic (they execute at the memory side), and would walk past a slot that
// holds its own key.  The walk is bounded by the pair's capacity and raises the error flag when it runs out; it cannot
// spin.  The count runs in a LATER launch -- the kernel boundary makes the bitmap visible to plain loads -- and reads the
// bitmap alone: one workgroup per pair, three popcounts per word, a fixed-order block sum (integers below 2^53 in fp64:
// exact), one store of {a, b, c}.  No float atomics, no inline assembly, no waiting on another workgroup.
//
// Workspace.  Pairs are processed in chunks whose tables together hold at most VOX_MAX_SLOTS = 2^25 slots: 256 MiB of keys
// plus 8 MiB of bitmap, whatever the call holds (RLDM_VOXEL_MAX_SLOTS in the header).  A single pair above that (more than
// 2^24 points on its two sides together) is an error through rldm_last_error.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)      // (+ -ffp-contract=off in the Makefile) c / v is a single IEEE operation

namespace {

constexpr int VOX_THREADS = 256;
constexpr int VOX_MIN_SLOTS = 16;                            // one bitmap word: every table starts on a word boundary
constexpr long long VOX_MAX_SLOTS = RLDM_VOXEL_MAX_SLOTS;    // slots of one chunk's tables together
constexpr int VOX_INSERT_WGS = 256 * 8;                      // grid cap of the insert kernel (it strides over the points)
constexpr float VOX_HALF = 1048576.0f;                       // 2^20
constexpr int VOX_ERR_RANGE = 1, VOX_ERR_FULL = 2;

__device__ inline unsigned long long vox_hash(unsigned long long k) {       // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    return k ^ (k >> 33);
}

// Element e of the chunk is point e of its packed x points when e < nx_chunk, else point e - nx_chunk of its y points.
// xoff / yoff point at the chunk's first pair (pairs + 1 entries each); tbase[p] is the first slot of pair p's table inside the
// chunk's allocation (a multiple of 16), tcap[p] its capacity (a power of two).
__global__ __launch_bounds__(VOX_THREADS) void voxel_insert_kernel(const float* __restrict__ x, const int* __restrict__ xoff,
                                                                   int xstride, const float* __restrict__ y,
                                                                   const int* __restrict__ yoff, int ystride, int pairs,
                                                                   const int* __restrict__ tbase, const int* __restrict__ tcap,
                                                                   float v, unsigned long long* __restrict__ table,
                                                                   unsigned* __restrict__ bitmap, int* __restrict__ err) {
    const int x0 = xoff[0], y0 = yoff[0];
    const int nx = xoff[pairs] - x0, total = nx + (yoff[pairs] - y0);
    for (int e = blockIdx.x * VOX_THREADS + threadIdx.x; e < total; e += gridDim.x * VOX_THREADS) {
        const int side = e >= nx;
        const int* off = side ? yoff : xoff;
        const int i = side ? y0 + (e - nx) : x0 + e;         // index into the packed points of its side
        const int lo = segment_of(off, pairs, i);
        const float* pt = side ? y + (size_t)i * ystride : x + (size_t)i * xstride;
        const float q0 = floorf(f_div(pt[0], v)), q1 = floorf(f_div(pt[1], v)), q2 = floorf(f_div(pt[2], v));
        if (!(q0 >= -VOX_HALF && q0 < VOX_HALF && q1 >= -VOX_HALF && q1 < VOX_HALF && q2 >= -VOX_HALF && q2 < VOX_HALF)) {
            atomicOr(err, VOX_ERR_RANGE);                    // (NaN fails every comparison)
            continue;
        }
        const unsigned long long key = (1ULL << 63) | (unsigned long long)((int)q0 + (1 << 20)) |
                                       (unsigned long long)((int)q1 + (1 << 20)) << 21 |
                                       (unsigned long long)((int)q2 + (1 << 20)) << 42;
        const unsigned base = (unsigned)tbase[lo], mask = (unsigned)tcap[lo] - 1u;
        unsigned slot = (unsigned)vox_hash(key) & mask;
        bool placed = false;
        for (unsigned probe = 0; probe <= mask; ++probe) {   // at most `capacity` slots: the walk cannot spin
            const unsigned long long old = atomicCAS(table + base + slot, 0ULL, key);
            if (old == 0ULL || old == key) {
                const unsigned s = base + slot;
                atomicOr(bitmap + (s >> 4), (1u << side) << ((s & 15u) * 2u));
                placed = true;
                break;
            }
            slot = (slot + 1u) & mask;
        }
        if (!placed) atomicOr(err, VOX_ERR_FULL);
    }
}

// one workgroup per pair of the chunk, launched after voxel_insert_kernel has ended; counts points at the chunk's first pair
__global__ __launch_bounds__(VOX_THREADS) void voxel_count_kernel(const unsigned* __restrict__ bitmap,
                                                                  const int* __restrict__ tbase, const int* __restrict__ tcap,
                                                                  int* __restrict__ counts) {
    __shared__ double sh[VOX_THREADS / 64];
    const int p = blockIdx.x;
    const unsigned* w = bitmap + ((unsigned)tbase[p] >> 4);
    const int words = tcap[p] >> 4;
    int a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < words; i += VOX_THREADS) {
        const unsigned m = w[i], in_x = m & 0x55555555u, in_y = (m >> 1) & 0x55555555u;
        a += __popc(in_x);
        b += __popc(in_y);
        c += __popc(in_x & in_y);
    }
    const double sa = block_sum((double)a, sh), sb = block_sum((double)b, sh), sc = block_sum((double)c, sh);
    if (threadIdx.x == 0) {
        counts[3 * p + 0] = (int)sa;
        counts[3 * p + 1] = (int)sb;
        counts[3 * p + 2] = (int)sc;
    }
}

}  // namespace

extern "C" {

int rldm_voxel_counts(const float* x, const int32_t* x_offsets, int x_stride, const float* y, const int32_t* y_offsets,
                      int y_stride, int num_pairs, float voxel, int32_t* counts, void* stream) {
    RLDM_REQUIRE(x && x_offsets && y && y_offsets && counts, "null argument");
    RLDM_REQUIRE(num_pairs > 0 && x_stride >= 3 && y_stride >= 3, "bad shape");
    RLDM_REQUIRE(voxel > 0.0f && std::isfinite(voxel), "voxel must be positive and finite");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> xo(num_pairs + 1), yo(num_pairs + 1);
    if (int rc = fetch_offsets(st, x_offsets, xo, y_offsets, yo)) return rc;
    // per pair: capacity, and the first slot of its table inside its chunk's allocation: [tbase: num_pairs][tcap: num_pairs]
    std::vector<int32_t> tab(2 * (size_t)num_pairs);
    int32_t* tbase = tab.data();
    int32_t* tcap = tab.data() + num_pairs;
    std::vector<int> chunk_first;                            // first pair of every chunk, then num_pairs
    long long used = 0, largest = 0;
    for (int p = 0; p < num_pairs; ++p) {
        const long long need = 2LL * ((long long)(xo[p + 1] - xo[p]) + (yo[p + 1] - yo[p]));
        if (need > VOX_MAX_SLOTS) {
            rldm::set_error("pair " + std::to_string(p) + " holds " + std::to_string(need / 2) + " points, above the " +
                            std::to_string(VOX_MAX_SLOTS / 2) + " one pair's voxel table takes");
            return 1;
        }
        long long cap = VOX_MIN_SLOTS;
        while (cap < need) cap *= 2;
        if (p == 0 || used + cap > VOX_MAX_SLOTS) {
            chunk_first.push_back(p);
            used = 0;
        }
        tbase[p] = (int32_t)used;
        tcap[p] = (int32_t)cap;
        used += cap;
        largest = std::max(largest, used);
    }
    chunk_first.push_back(num_pairs);

    DevBuf tbuf(st), kbuf(st), bbuf(st), ebuf(st);
    RLDM_HIP_CHECK(tbuf.alloc(tab.size() * sizeof(int32_t)));
    RLDM_HIP_CHECK(kbuf.alloc((size_t)largest * sizeof(unsigned long long)));
    RLDM_HIP_CHECK(bbuf.alloc((size_t)(largest / 16) * sizeof(unsigned)));
    RLDM_HIP_CHECK(ebuf.alloc(sizeof(int)));
    const int32_t* dbase = tbuf.as<int32_t>();
    const int32_t* dcap = dbase + num_pairs;
    unsigned long long* table = kbuf.as<unsigned long long>();
    unsigned* bitmap = bbuf.as<unsigned>();
    int* err = ebuf.as<int>();
    RLDM_HIP_CHECK(hipMemcpyAsync(tbuf.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RLDM_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int), st));
    for (size_t c = 0; c + 1 < chunk_first.size(); ++c) {    // one after the other on the stream: they share the tables
        const int p0 = chunk_first[c], pairs = chunk_first[c + 1] - p0;
        const long long slots = (long long)tbase[p0 + pairs - 1] + tcap[p0 + pairs - 1];
        const long long points = (long long)(xo[p0 + pairs] - xo[p0]) + (yo[p0 + pairs] - yo[p0]);      // <= slots / 2
        RLDM_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)slots * sizeof(unsigned long long), st));
        RLDM_HIP_CHECK(hipMemsetAsync(bitmap, 0, (size_t)(slots / 16) * sizeof(unsigned), st));
        const int grid = (int)std::min<long long>((points + VOX_THREADS - 1) / VOX_THREADS, VOX_INSERT_WGS);
        voxel_insert_kernel<<<grid, VOX_THREADS, 0, st>>>(x, x_offsets + p0, x_stride, y, y_offsets + p0, y_stride, pairs,
                                                          dbase + p0, dcap + p0, voxel, table, bitmap, err);
        RLDM_HIP_CHECK(hipGetLastError());
        voxel_count_kernel<<<pairs, VOX_THREADS, 0, st>>>(bitmap, dbase + p0, dcap + p0, counts + 3 * (size_t)p0);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    int flagged = 0;
    RLDM_HIP_CHECK(hipMemcpyAsync(&flagged, err, sizeof(int), hipMemcpyDeviceToHost, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));              // also: `tab` (pageable host memory) must outlive its upload
    if (flagged) {                                           // nothing is reported: the counts of such a call are cleared
        RLDM_HIP_CHECK(hipMemsetAsync(counts, 0, 3 * (size_t)num_pairs * sizeof(int32_t), st));
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        if (flagged & VOX_ERR_RANGE) {
            rldm::set_error("a point is out of range: a coordinate is NaN or inf, or floor(c / voxel) lies outside [-2^20, 2^20)");
            return RLDM_VOXEL_RANGE;
        }
        rldm::set_error("a voxel table filled up (internal error: a table holds twice its pair's points)");
        return 1;
    }
    return 0;
}

}  // extern "C"
