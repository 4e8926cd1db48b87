// lidar.hip -- range image <-> point cloud on gfx950: the step right after the sampler in
// every reference driver (ldm/inference.py:171-183) and the one right before the training path (ldm/dataset.py:159-226).
//
// Everything here is HBM / atomic bound, fp32, one thread per range-image pixel or per LiDAR return:
//   range_to_points_kernel   point_cloud_to_range_image.to_pc_torch          ldm/dataset.py:228-278
//   bev_splat_kernel         to_voxel + _splat_points_to_volumes (votes)     ldm/dataset.py:280-288, 13-124
//   bev_finalize_kernel      feature / clamp(density), log(density + 1)      ldm/dataset.py:126-130, 289-293
//   bev_finalize_train / bev_cell_grad / bev_pixel_grad   to_voxel for training: raw accumulators kept, the backward a gather
//                                                         (vae/sgm/modules/autoencoding/losses: disc_bev, bev_rec_weight)
//   bev_votes / radix_hist / radix_scan / radix_scatter / bev_segments / bev_ordered_sum   the order-fixed splat: votes sorted by
//                                                         cell (stable), each cell summed left to right; no fp32 atomics
//   filter_count / filter_scatter   `pc[norm(pc[:, :3]) < 90]` in order      ldm/inference.py:177-179
//   render_u8_kernel         `(x.permute(2,1,0).clip(0,1)*255).astype(u8)`   ldm/inference.py:180-183
//   project_* kernels        point_cloud_to_range_image.__call__ + process_miss_value + normalize
//                                                                            ldm/dataset.py:159-226
// The arithmetic keeps the reference's fp32 operation order (no FMA contraction) so cell indices and the ordered
// compaction agree with the torch/numpy result wherever the inputs do.
#include "eval_common.h"
#include "../../include/rangeldm_hip.h"

#include <cmath>
#include <map>
#include <vector>

#pragma clang fp contract(off)      // and -ffp-contract=off for this file in the Makefile (covers the header inlines and
                                    // eval_common.h's f_mul / f_add / f_sub / f_div / f_sqrt, which the arithmetic here uses)

namespace {

struct LidarDev {
    const float* cos_incl;
    const float* sin_incl;
    const float* incl;
    const float* height;
    int H;
    int mode;          // 0 linear, 1 log, 2 inverse
    float mean, std, range_fill, intensity_fill;
};

// the decoded range before `r_true[r_true < 0] = range_fill` (ldm/dataset.py:240-245)
__device__ inline float decode_range_raw(float v, const LidarDev& L) {
    float r;
    if (L.mode == 1) r = f_sub(exp2f(f_mul(v, 6.f)), 1.f);
    else if (L.mode == 2) r = f_div(1.f, fmaxf(v, 0.0001f));
    else r = f_add(f_mul(v, L.std), L.mean);
    return r;
}

__device__ inline float decode_range(float v, const LidarDev& L) {
    const float r = decode_range_raw(v, L);
    return r < 0.f ? L.range_fill : r;
}

// pixel (w, h) with decoded range r -> sensor-frame xyz (ldm/dataset.py:251-272)
__device__ inline void pixel_to_xyz(float r, int w, int h, const LidarDev& L, const float* cos_azi, const float* sin_azi,
                                    float* x, float* y, float* z) {
    const float xy = f_mul(r, L.cos_incl[h]);
    *z = f_sub(L.height[h], f_mul(r, L.sin_incl[h]));
    *x = f_mul(xy, cos_azi[w]);
    *y = f_mul(xy, sin_azi[w]);
}

// ---- to_pc_torch ------------------------------------------------------------------------------------------------
// img (B, C, W, H): flat pixel index n = w * H + h is also the point index of the reference's reshape(B, -1).
__global__ __launch_bounds__(256) void range_to_points_kernel(const float* __restrict__ img, int C, int W, int H,
                                                              LidarDev L, const float* __restrict__ cos_azi,
                                                              const float* __restrict__ sin_azi, float* __restrict__ pts) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int N = W * H;
    if (n >= N) return;
    const float* im = img + (size_t)b * C * N;
    const float r = decode_range(im[n], L);
    float x, y, z;
    pixel_to_xyz(r, n / H, n % H, L, cos_azi, sin_azi, &x, &y, &z);
    if (C > 1) {
        reinterpret_cast<float4*>(pts)[(size_t)b * N + n] = make_float4(x, y, z, im[N + n]);
    } else {
        float* p = pts + ((size_t)b * N + n) * 3;
        p[0] = x; p[1] = y; p[2] = z;
    }
}

// ---- to_voxel ---------------------------------------------------------------------------------------------------
struct GridDev {
    int gx, gy, gz;            // grid_sizes = [gz, gy, gx]
    float cx, cy, cz;          // (hi + lo) / 2
    float hx, hy, hz;          // (hi - lo) / 2
};

__device__ inline float grid_coord(float v, float c, float h, int g) {
    const float p = f_div(f_sub(v, c), h);
    return f_mul(f_mul(f_add(p, 1.f), 0.5f), (float)(g - 1));
}

// One thread per pixel: decode, project, cast its 8 trilinear votes with hardware fp32 atomics straight into the
// (B, 2*gz, gy, gx) output (density planes first, then feature planes).  Out-of-volume votes carry weight 0 in the
// reference (added to a random voxel): they are dropped.
__global__ __launch_bounds__(256) void bev_splat_kernel(const float* __restrict__ img, int C, int W, int H, LidarDev L,
                                                        const float* __restrict__ cos_azi, const float* __restrict__ sin_azi,
                                                        GridDev G, float* __restrict__ vox) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int N = W * H;
    if (n >= N) return;
    const float* im = img + (size_t)b * C * N;
    const float r = decode_range(im[n], L);
    const float f = im[N + n];
    float x, y, z;
    pixel_to_xyz(r, n / H, n % H, L, cos_azi, sin_azi, &x, &y, &z);
    const float px = grid_coord(x, G.cx, G.hx, G.gx), py = grid_coord(y, G.cy, G.hy, G.gy), pz = grid_coord(z, G.cz, G.hz, G.gz);
    // anything that cannot touch the volume (also NaN) is dropped before the float -> int conversion
    if (!(px > -1.f && px < (float)G.gx && py > -1.f && py < (float)G.gy && pz > -1.f && pz < (float)G.gz)) return;
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    const int X = (int)fx, Y = (int)fy, Z = (int)fz;
    const float rx = f_sub(px, fx), ry = f_sub(py, fy), rz = f_sub(pz, fz);
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    float* dens = vox + (size_t)b * 2 * nvox;
    float* feat = dens + nvox;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        const int X_ = X + dx;
        const float wx = dx ? rx : f_sub(1.f, rx);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int Y_ = Y + dy;
            const float wy = dy ? ry : f_sub(1.f, ry);
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const int Z_ = Z + dz;
                const float wz = dz ? rz : f_sub(1.f, rz);
                const float w = f_mul(f_mul(wx, wy), wz);
                const bool ok = X_ >= 0 && X_ < G.gx && Y_ >= 0 && Y_ < G.gy && Z_ >= 0 && Z_ < G.gz;
                if (ok && w != 0.f) {
                    const size_t idx = ((size_t)Z_ * G.gy + Y_) * G.gx + X_;
                    unsafeAtomicAdd(dens + idx, w);
                    unsafeAtomicAdd(feat + idx, f_mul(w, f));
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void bev_finalize_kernel(float* __restrict__ vox, size_t nvox, int log_density,
                                                           float min_weight) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= nvox) return;
    float* dens = vox + (size_t)b * 2 * nvox;
    float* feat = dens + nvox;
    const float d = dens[i];
    if (d == 0.f) return;               // no votes: feature 0 / min_weight = 0 and log(0 + 1) = 0 are already there
    feat[i] = f_div(feat[i], fmaxf(d, min_weight));
    if (log_density) dens[i] = logf(f_add(d, 1.f));
}

// ---- to_voxel for training: the raw accumulators are kept, the backward is a gather --------------------------------
// bev_finalize_kernel out of place: raw (B, 2*gz, gy, gx) = (d | S) stays as the splat left it, vox takes the bits
// rldm_lidar_to_voxel writes (an empty cell: 0 and 0).
__global__ __launch_bounds__(256) void bev_finalize_train_kernel(const float* __restrict__ raw, float* __restrict__ vox,
                                                                 size_t nvox, int log_density, float min_weight) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= nvox) return;
    const float* rd = raw + (size_t)b * 2 * nvox;
    float* dens = vox + (size_t)b * 2 * nvox;
    const float d = rd[i], S = rd[nvox + i];
    if (d == 0.f) { dens[i] = d; dens[nvox + i] = S; return; }
    dens[nvox + i] = f_div(S, fmaxf(d, min_weight));
    dens[i] = log_density ? logf(f_add(d, 1.f)) : d;
}

// Backward, launch 1, one thread per cell: the finalise step's derivative.  With gD, gF the upstream gradients of the two
// output planes:  a = d(loss) / d(d) = gD / (d + 1) [log] or gD, minus [d >= min_weight] gF S / d^2 (clamp(min) passes the
// gradient where d >= min);  e = d(loss) / d(S) = gF / max(d, min_weight).  cg (B, 2*gz, gy, gx) = (a | e).
__global__ __launch_bounds__(256) void bev_cell_grad_kernel(const float* __restrict__ raw, const float* __restrict__ dvox,
                                                            float* __restrict__ cg, size_t nvox, int log_density,
                                                            float min_weight) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= nvox) return;
    const size_t o = (size_t)b * 2 * nvox;
    const float d = raw[o + i], S = raw[o + nvox + i];
    const float gD = dvox[o + i], gF = dvox[o + nvox + i];
    float a = log_density ? f_div(gD, f_add(d, 1.f)) : gD;
    if (d >= min_weight) a = f_sub(a, f_div(f_mul(gF, S), f_mul(d, d)));
    cg[o + i] = a;
    cg[o + nvox + i] = f_div(gF, fmaxf(d, min_weight));
}

// Backward, launch 2, one thread per pixel: the pixel recomputes its cell, remainders and in-grid tests with the forward's own
// expressions and GATHERS from cg -- no atomics.  A vote of weight 0 whose cell is inside the grid is included: its
// weight's derivative is not 0.  dimg (B, 2, W, H): channel 0 = d / d(range value), channel 1 = d / d(remission).
// A pixel the forward dropped gets 0 in both; one whose decoded range was negative (replaced by range_fill, a constant) gets 0
// in channel 0 and, should the fill point lie inside the volume, its remission gradient in channel 1.
__global__ __launch_bounds__(256) void bev_pixel_grad_kernel(const float* __restrict__ img, int C, int W, int H, LidarDev L,
                                                             const float* __restrict__ cos_azi, const float* __restrict__ sin_azi,
                                                             GridDev G, const float* __restrict__ cg, float* __restrict__ dimg) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int N = W * H;
    if (n >= N) return;
    const float* im = img + (size_t)b * C * N;
    float* out = dimg + (size_t)b * 2 * N;
    const float v = im[n];
    const float r = decode_range(v, L);
    const float f = im[N + n];
    const int w_ = n / H, h_ = n % H;
    float x, y, z;
    pixel_to_xyz(r, w_, h_, L, cos_azi, sin_azi, &x, &y, &z);
    const float px = grid_coord(x, G.cx, G.hx, G.gx), py = grid_coord(y, G.cy, G.hy, G.gy), pz = grid_coord(z, G.cz, G.hz, G.gz);
    if (!(px > -1.f && px < (float)G.gx && py > -1.f && py < (float)G.gy && pz > -1.f && pz < (float)G.gz)) {
        out[n] = 0.f;
        out[N + n] = 0.f;
        return;
    }
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    const int X = (int)fx, Y = (int)fy, Z = (int)fz;
    const float rx = f_sub(px, fx), ry = f_sub(py, fy), rz = f_sub(pz, fz);
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    const float* A = cg + (size_t)b * 2 * nvox;
    const float* E = A + nvox;
    float df = 0.f, dpx = 0.f, dpy = 0.f, dpz = 0.f;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        const int X_ = X + dx;
        const float wx = dx ? rx : f_sub(1.f, rx);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int Y_ = Y + dy;
            const float wy = dy ? ry : f_sub(1.f, ry);
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const int Z_ = Z + dz;
                const float wz = dz ? rz : f_sub(1.f, rz);
                const bool ok = X_ >= 0 && X_ < G.gx && Y_ >= 0 && Y_ < G.gy && Z_ >= 0 && Z_ < G.gz;
                if (ok) {
                    const size_t idx = ((size_t)Z_ * G.gy + Y_) * G.gx + X_;
                    const float e = E[idx];
                    const float q = f_add(A[idx], f_mul(f, e));
                    df = f_add(df, f_mul(f_mul(f_mul(wx, wy), wz), e));
                    const float tx = f_mul(q, f_mul(wy, wz)), ty = f_mul(q, f_mul(wx, wz)), tz = f_mul(q, f_mul(wx, wy));
                    dpx = dx ? f_add(dpx, tx) : f_sub(dpx, tx);
                    dpy = dy ? f_add(dpy, ty) : f_sub(dpy, ty);
                    dpz = dz ? f_add(dpz, tz) : f_sub(dpz, tz);
                }
            }
        }
    }
    // d(range) / d(value); 0 where the decoded range was replaced by the constant range_fill
    float drdv;
    if (decode_range_raw(v, L) < 0.f) drdv = 0.f;
    else if (L.mode == 1) drdv = f_mul(4.1588830833596715f, exp2f(f_mul(v, 6.f)));          // 6 ln 2
    else if (L.mode == 2) drdv = v > 0.0001f ? f_div(-1.f, f_mul(v, v)) : 0.f;
    else drdv = L.std;
    const float kx = f_div(f_mul(0.5f, (float)(G.gx - 1)), G.hx), ky = f_div(f_mul(0.5f, (float)(G.gy - 1)), G.hy),
                kz = f_div(f_mul(0.5f, (float)(G.gz - 1)), G.hz);
    const float ci = L.cos_incl[h_], si = L.sin_incl[h_];
    const float gx_ = f_mul(f_mul(f_mul(dpx, kx), ci), cos_azi[w_]);
    const float gy_ = f_mul(f_mul(f_mul(dpy, ky), ci), sin_azi[w_]);
    const float gz_ = f_mul(f_mul(dpz, kz), si);
    out[n] = f_mul(f_sub(f_add(gx_, gy_), gz_), drdv);
    out[N + n] = df;
}

// ---- order-fixed to_voxel: every cell is the fp32 sum of its votes in ascending vote id -------------------------------
// A vote has the id v = n * 8 + (dx * 4 + dy * 2 + dz).  The votes are written out at position v, sorted by cell with a STABLE
// LSD radix sort (a pixel votes at most once into a cell, so within a cell ascending v is what a stable sort of votes that start
// in v order leaves), and each cell then adds its segment left to right: d = ((0 + w_1) + w_2) + .., S the same over f_mul(w, f).
// No floating-point atomic anywhere; no workgroup waits on another (every histogram, scan and scatter is its own launch).
//
// The sort's unit is a CHUNK of ORD_CHUNK consecutive positions, owned by one wave, which walks it in ORD_CHUNK / 64 rounds of 64;
// a workgroup is four independent waves (four chunks).  Per 8-bit digit pass: radix_hist (per-chunk digit counts -> table
// [digit][chunk]), radix_scan (one wave per image and digit: exclusive scan of that digit's row, and its total), radix_scatter
// (start of the digit = the totals below it; rank inside the round from __ballot masks, base from the wave's running per-digit
// counters in LDS -- never from an atomic's return value).
constexpr int ORD_CHUNK = 1024;             // positions per wave
constexpr int ORD_ROUNDS = ORD_CHUNK / 64;
constexpr int ORD_SHORT = 16;               // segments up to this long are added by their cell's own lane (bev_ordered_sum_kernel)
constexpr int ORD_LOADS = 4;                // 64-vote loads a wave keeps in flight while it adds a long segment

// One thread per pixel: bev_splat_kernel's votes, written instead of cast.  keys[v] = the cell, or nvox (the sentinel, sorted
// behind every cell) for a vote the atomic kernel would not cast; vals[v] = (w, w f), read only where the key is a cell.
__global__ __launch_bounds__(256) void bev_votes_kernel(const float* __restrict__ img, int C, int W, int H, LidarDev L,
                                                        const float* __restrict__ cos_azi, const float* __restrict__ sin_azi,
                                                        GridDev G, unsigned* __restrict__ keys, float2* __restrict__ vals) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int N = W * H;
    if (n >= N) return;
    const size_t M = (size_t)N * 8;
    const unsigned nvox = (unsigned)((size_t)G.gz * G.gy * G.gx);
    const float* im = img + (size_t)b * C * N;
    unsigned k[8];
    float2 wv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { k[c] = nvox; wv[c] = make_float2(0.f, 0.f); }
    const float r = decode_range(im[n], L);
    const float f = im[N + n];
    float x, y, z;
    pixel_to_xyz(r, n / H, n % H, L, cos_azi, sin_azi, &x, &y, &z);
    const float px = grid_coord(x, G.cx, G.hx, G.gx), py = grid_coord(y, G.cy, G.hy, G.gy), pz = grid_coord(z, G.cz, G.hz, G.gz);
    if (px > -1.f && px < (float)G.gx && py > -1.f && py < (float)G.gy && pz > -1.f && pz < (float)G.gz) {
        const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
        const int X = (int)fx, Y = (int)fy, Z = (int)fz;
        const float rx = f_sub(px, fx), ry = f_sub(py, fy), rz = f_sub(pz, fz);
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int X_ = X + dx;
            const float wx = dx ? rx : f_sub(1.f, rx);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int Y_ = Y + dy;
                const float wy = dy ? ry : f_sub(1.f, ry);
#pragma unroll
                for (int dz = 0; dz < 2; ++dz) {
                    const int Z_ = Z + dz;
                    const float wz = dz ? rz : f_sub(1.f, rz);
                    const float w = f_mul(f_mul(wx, wy), wz);
                    const bool ok = X_ >= 0 && X_ < G.gx && Y_ >= 0 && Y_ < G.gy && Z_ >= 0 && Z_ < G.gz;
                    if (ok && w != 0.f) {
                        k[dx * 4 + dy * 2 + dz] = (unsigned)(((size_t)Z_ * G.gy + Y_) * G.gx + X_);
                        wv[dx * 4 + dy * 2 + dz] = make_float2(w, f_mul(w, f));
                    }
                }
            }
        }
    }
    uint4* ko = reinterpret_cast<uint4*>(keys + (size_t)b * M + (size_t)n * 8);
    ko[0] = make_uint4(k[0], k[1], k[2], k[3]);
    ko[1] = make_uint4(k[4], k[5], k[6], k[7]);
    float4* vo = reinterpret_cast<float4*>(vals + (size_t)b * M + (size_t)n * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) vo[c] = make_float4(wv[2 * c].x, wv[2 * c].y, wv[2 * c + 1].x, wv[2 * c + 1].y);
}

// Digit counts of every chunk: table[b][digit * nchunks + chunk].  The LDS integer atomics' return values are not used.
__global__ __launch_bounds__(256) void radix_hist_kernel(const unsigned* __restrict__ keys, int M, int nchunks, int shift,
                                                         int* __restrict__ table) {
    __shared__ int cnt[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + wave;
    const int b = blockIdx.y;
#pragma unroll
    for (int d = lane; d < 256; d += 64) cnt[wave][d] = 0;
    __syncthreads();
    const unsigned* kb = keys + (size_t)b * M;
    for (int r = 0; r < ORD_ROUNDS; ++r) {
        const long long i = (long long)chunk * ORD_CHUNK + r * 64 + lane;
        if (i < M) atomicAdd(&cnt[wave][(kb[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    if (chunk < nchunks) {
        int* tb = table + (size_t)b * 256 * nchunks;
#pragma unroll
        for (int d = lane; d < 256; d += 64) tb[(size_t)d * nchunks + chunk] = cnt[wave][d];
    }
}

// inclusive scan over the 64 lanes of a wave
__device__ inline int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(v, off);
        if (lane >= off) v += up;
    }
    return v;
}

// One wave per (image, digit): the digit's row of the table, nchunks counts, becomes its exclusive scan in place (64 entries a step,
// coalesced, the carry in a register) and the row's total goes to totals[b][digit].  radix_scatter adds the digits below.
__global__ __launch_bounds__(256) void radix_scan_kernel(int* __restrict__ table, int nchunks, int* __restrict__ totals) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int digit = blockIdx.x * 4 + wave;
    const int b = blockIdx.y;
    int* row = table + ((size_t)b * 256 + digit) * nchunks;
    int carry = 0;
    for (int base = 0; base < nchunks; base += 64) {
        const int i = base + lane;
        const int c = i < nchunks ? row[i] : 0;
        const int incl = wave_scan_incl(c, lane);
        if (i < nchunks) row[i] = carry + incl - c;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) totals[b * 256 + digit] = carry;
}

// Stable scatter of one digit pass.  ids_in == nullptr: the first pass, where position i holds vote i.  Per round of 64 the lanes
// that share a digit are found with eight ballots; a lane's place is its wave's running count of that digit (LDS, started from
// the scanned table) plus the number of such lanes below it; the lowest of them then moves the count on.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const unsigned* __restrict__ keys_in, const int* __restrict__ ids_in,
                                                            int M, int nchunks, int shift, const int* __restrict__ table,
                                                            const int* __restrict__ totals, unsigned* __restrict__ keys_out,
                                                            int* __restrict__ ids_out) {
    __shared__ int base[4][256];
    __shared__ int first[256];              // where the image's votes of digit d start: the totals of the digits below d
    __shared__ int wave_tot[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + wave;
    const int b = blockIdx.y;
    {
        const int c = totals[b * 256 + threadIdx.x];
        const int incl = wave_scan_incl(c, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int below = 0;
        for (int w = 0; w < wave; ++w) below += wave_tot[w];
        first[threadIdx.x] = below + incl - c;
    }
    __syncthreads();
    if (chunk < nchunks) {
        const int* tb = table + (size_t)b * 256 * nchunks;
#pragma unroll
        for (int d = lane; d < 256; d += 64) base[wave][d] = first[d] + tb[(size_t)d * nchunks + chunk];
    }
    __syncthreads();
    const size_t o = (size_t)b * M;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < ORD_ROUNDS; ++r) {
        const long long i = (long long)chunk * ORD_CHUNK + r * 64 + lane;
        const bool valid = i < M;
        const unsigned key = valid ? keys_in[o + i] : 0u;
        const int id = valid ? (ids_in ? ids_in[o + i] : (int)i) : 0;
        const unsigned digit = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long m = __ballot((digit >> bit) & 1u);
            same &= ((digit >> bit) & 1u) ? m : ~m;
        }
        int pos = 0;
        if (valid) pos = base[wave][digit] + __popcll(same & below);
        __syncthreads();                                    // every lane has read its count before the lowest lane moves it
        if (valid && (same & below) == 0ull) base[wave][digit] += __popcll(same);
        __syncthreads();
        if (valid) {
            keys_out[o + pos] = key;
            ids_out[o + pos] = id;
        }
    }
}

// seg[b][cell] = (first, one past last) position of the cell's votes in the sorted order; cleared to (0, 0) before the launch.
__global__ __launch_bounds__(256) void bev_segments_kernel(const unsigned* __restrict__ keys, int M, unsigned nvox,
                                                           int2* __restrict__ seg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= M) return;
    const unsigned* kb = keys + (size_t)b * M;
    int2* sb = seg + (size_t)b * nvox;
    const unsigned k = kb[i];
    if (i == 0) {
        if (k < nvox) sb[k].x = 0;
    } else {
        const unsigned kp = kb[i - 1];
        if (k != kp) {
            if (k < nvox) sb[k].x = (int)i;
            if (kp < nvox) sb[kp].y = (int)i;
        }
    }
    if (i == M - 1 && k < nvox) sb[k].y = M;
}

// a += v.x, q += v.y of lanes 0 .. cnt - 1, one lane after the other (cnt <= 0: nothing); every lane of the wave ends with the same sums
__device__ inline void add_lanes_in_order(float2 v, int cnt, float& a, float& q) {
    const int x = __float_as_int(v.x), y = __float_as_int(v.y);
    if (cnt >= 64) {
#pragma unroll
        for (int t = 0; t < 64; ++t) {
            a = f_add(a, __int_as_float(__builtin_amdgcn_readlane(x, t)));
            q = f_add(q, __int_as_float(__builtin_amdgcn_readlane(y, t)));
        }
    } else {
        for (int t = 0; t < cnt; ++t) {
            a = f_add(a, __int_as_float(__builtin_amdgcn_readlane(x, t)));
            q = f_add(q, __int_as_float(__builtin_amdgcn_readlane(y, t)));
        }
    }
}

// One thread per cell writes raw = (d | S): 0.f, then one fp32 addition per vote of the cell's segment, left to right.  A segment
// of up to ORD_SHORT votes is read by the cell's own lane.  A longer one (every pixel that decodes to a range near 0 votes into
// the few cells under the sensor) is read by the whole wave, 64 votes a load, the next ORD_LOADS loads in flight while the values
// of the current ones are handed lane by lane to the one running sum -- the same additions in the same order.
__global__ __launch_bounds__(256) void bev_ordered_sum_kernel(const int2* __restrict__ seg, const int* __restrict__ ids,
                                                              const float2* __restrict__ vals, int M, unsigned nvox,
                                                              float* __restrict__ raw) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int* ib = ids + (size_t)b * M;
    const float2* vb = vals + (size_t)b * M;
    const int2 se = c < nvox ? seg[(size_t)b * nvox + c] : make_int2(0, 0);
    const int len = se.y - se.x;
    float d = 0.f, S = 0.f;
    if (len <= ORD_SHORT) {
        for (int j = se.x; j < se.y; ++j) {
            const float2 v = vb[ib[j]];
            d = f_add(d, v.x);
            S = f_add(S, v.y);
        }
    }
    unsigned long long todo = __ballot(len > ORD_SHORT);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int s0 = __builtin_amdgcn_readlane(se.x, src), e0 = __builtin_amdgcn_readlane(se.y, src);
        float a = 0.f, q = 0.f;
        float2 cur[ORD_LOADS], nxt[ORD_LOADS];
#pragma unroll
        for (int g = 0; g < ORD_LOADS; ++g) {
            const long long i = (long long)s0 + g * 64 + lane;
            cur[g] = i < e0 ? vb[ib[i]] : make_float2(0.f, 0.f);
        }
        for (long long j = s0; j < e0; j += 64 * ORD_LOADS) {
#pragma unroll
            for (int g = 0; g < ORD_LOADS; ++g) {
                const long long i = j + (ORD_LOADS + g) * 64 + lane;
                nxt[g] = i < e0 ? vb[ib[i]] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int g = 0; g < ORD_LOADS; ++g) {
                add_lanes_in_order(cur[g], (int)min(64ll, e0 - (j + g * 64)), a, q);
                cur[g] = nxt[g];
            }
        }
        if (lane == src) { d = a; S = q; }
    }
    if (c < nvox) {
        float* rb = raw + (size_t)b * 2 * nvox;
        rb[c] = d;
        rb[(size_t)nvox + c] = S;
    }
}

// ---- ordered depth filter ---------------------------------------------------------------------------------------
// pass 1: kept points per 256-point chunk; pass 2: chunk base = sum of the preceding counts, wave ballots give the
// rank inside the chunk.  The kept points keep their order (what `pc[mask]` does), no atomics.
__device__ inline bool keep_point(const float* __restrict__ p, float max_depth) {
    const float d2 = f_add(f_add(f_mul(p[0], p[0]), f_mul(p[1], p[1])), f_mul(p[2], p[2]));
    return f_sqrt(d2) < max_depth;
}

__global__ __launch_bounds__(256) void filter_count_kernel(const float* __restrict__ pts, int N, int cols, float max_depth,
                                                           int* __restrict__ chunk_counts) {
    __shared__ int wave_cnt[4];
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const bool keep = n < N && keep_point(pts + ((size_t)b * N + n) * cols, max_depth);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) chunk_counts[(size_t)b * gridDim.x + blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ __launch_bounds__(256) void filter_scatter_kernel(const float* __restrict__ pts, int N, int cols, float max_depth,
                                                             const int* __restrict__ chunk_counts, float* __restrict__ out,
                                                             int* __restrict__ counts) {
    __shared__ int red[4];
    __shared__ int wave_cnt[4];
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int* cc = chunk_counts + (size_t)b * nchunks;
    int part = 0;
    for (int i = threadIdx.x; i < chunk; i += 256) part += cc[i];
    for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
    const int n = chunk * 256 + threadIdx.x;
    const float* p = pts + ((size_t)b * N + n) * cols;
    const bool keep = n < N && keep_point(p, max_depth);
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv] = part; wave_cnt[wv] = __popcll(m); }
    __syncthreads();
    int base = red[0] + red[1] + red[2] + red[3];
    for (int i = 0; i < wv; ++i) base += wave_cnt[i];
    if (keep) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        float* q = out + ((size_t)b * N + pos) * cols;
        if (cols == 4) *reinterpret_cast<float4*>(q) = *reinterpret_cast<const float4*>(p);
        else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
    }
    if (chunk == nchunks - 1 && threadIdx.x == 0)
        counts[b] = red[0] + red[1] + red[2] + red[3] + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// ---- 8-bit rendering --------------------------------------------------------------------------------------------
// src (B, C, W, H) fp32, channel c -> dst [B][H][W] bytes: a 64 x 64 tile is read along H and written along W.
__global__ __launch_bounds__(256) void render_u8_kernel(const float* __restrict__ src, int C, int W, int H, int c,
                                                        unsigned char* __restrict__ dst) {
    __shared__ unsigned char tile[64][65];
    const int b = blockIdx.z, w0 = blockIdx.x * 64, h0 = blockIdx.y * 64;
    const float* s = src + ((size_t)b * C + c) * W * H;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int w = w0 + i, h = h0 + tx;
        if (w < W && h < H) {
            const float v = fminf(fmaxf(s[(size_t)w * H + h], 0.f), 1.f);
            tile[i][tx] = (unsigned char)(int)f_mul(v, 255.f);
        }
    }
    __syncthreads();
    unsigned char* d = dst + (size_t)b * W * H;
    for (int i = ty; i < 64; i += 4) {
        const int h = h0 + i, w = w0 + tx;
        if (w < W && h < H) d[(size_t)h * W + w] = tile[tx][i];
    }
}

// ---- projection (dataset side) ----------------------------------------------------------------------------------
// A LiDAR return competes for its pixel with a 64-bit key (range bits << 32 | point index): the reference writes the
// points sorted farthest-first so the NEAREST return of a pixel survives (ldm/dataset.py:173-185); atomicMin on the key
// yields the same winner without a sort (positive floats order like their bit patterns; equal ranges: the highest point
// index wins, which is what a stable farthest-first sort followed by in-order writes gives).
__global__ __launch_bounds__(256) void project_keys_kernel(const float* __restrict__ pts, int n_pts, int stride,
                                                           const int* __restrict__ rows, LidarDev L, int W, float min_depth,
                                                           unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pts) return;
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    if (min_depth > 0.f) {      // nuScenes: drop returns closer than 2 m (ldm/nuscenes_range_image.py:37-41)
        const float d = f_sqrt(f_add(f_add(f_mul(x, x), f_mul(y, y)), f_mul(z, z)));
        if (!(d > min_depth)) return;
    }
    int row;
    if (rows) {
        row = rows[i];
    } else {                    // ldm/kitti360_range_image.py:51-61: beam with the closest inclination
        const float xy = f_sqrt(f_add(f_mul(x, x), f_mul(y, y)));
        float best = INFINITY;
        row = 0;
        for (int h = 0; h < L.H; ++h) {
            const float e = fabsf(f_sub(L.incl[h], atan2f(f_sub(L.height[h], z), xy)));
            if (e < best) { best = e; row = h; }
        }
    }
    if (row < 0 || row >= L.H) return;
    // column (ldm/dataset.py:162-166): fp32 throughout (python scalars do not promote a float32 array), round half to even
    const float turn = f_div(f_add(atan2f(y, x), (float)M_PI), (float)(2.0 * M_PI));
    const float colf = f_sub((float)((double)W - 1.0 + 0.5), f_mul(turn, (float)W));
    int col = (int)rintf(colf);
    if (col == W) col = W - 1;
    if (col < 0) col = 0;
    const float zz = f_sub(z, L.height[row]);
    float rng = f_sqrt(f_add(f_add(f_mul(x, x), f_mul(y, y)), f_mul(zz, zz)));
    if (rng > L.range_fill) rng = L.range_fill;
    const unsigned long long key = ((unsigned long long)__float_as_uint(rng) << 32) | (unsigned int)~i;
    atomicMin(keys + (size_t)row * W + col, key);
}

// keys -> (H, W, 2) raw range image with -1 where no return landed
__global__ __launch_bounds__(256) void project_gather_kernel(const unsigned long long* __restrict__ keys,
                                                             const float* __restrict__ pts, int stride, LidarDev L, int W,
                                                             float2* __restrict__ raw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.H * W) return;
    const unsigned long long k = keys[i];
    float2 v = make_float2(-1.f, -1.f);
    if (k != ~0ull) {
        const float rng = __uint_as_float((unsigned int)(k >> 32));
        float val = rng;
        if (L.mode == 1) val = f_div(log2f(f_add(rng, 1.f)), 6.f);
        else if (L.mode == 2) val = f_div(1.f, rng);
        v = make_float2(val, pts[(size_t)(~(unsigned int)k) * stride + 3]);
    }
    raw[i] = v;
}

// process_miss_value + normalize + the (2, 1, 0) permute: raw (H, W, 2) -> image (2, W, H), mask (W, H), car (W, H)
__global__ __launch_bounds__(256) void project_finish_kernel(const float2* __restrict__ raw, LidarDev L, int W,
                                                             float fill0, float fill1, float* __restrict__ img,
                                                             unsigned char* __restrict__ mask, unsigned char* __restrict__ car) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int H = L.H;
    if (i >= H * W) return;
    const int w = i / H, h = i % H;         // output-major indexing: writes are contiguous along H
    auto filled = [&](int hh, int ww) -> float2 {      // after fill_noise: a missing pixel takes its right neighbour
        float2 v = raw[(size_t)hh * W + ww];
        if (v.x == -1.f) v = raw[(size_t)hh * W + (ww + 1 == W ? 0 : ww + 1)];
        return v;
    };
    float2 v = filled(h, w);
    // mask = (range > 0) of the pixel itself, or of the right neighbour where the pixel was missing
    const bool m = v.x > 0.f;
    const bool still = v.x == -1.f;
    bool cw = false;
    if (still) {
        const int hd = (h - 2 + H) % H, hu = (h + 2) % H, wr = (w - 2 + W) % W, wl = (w + 2) % W;
        cw = filled(hd, w).x != -1.f || filled(hu, w).x != -1.f || filled(h, wr).x != -1.f || filled(h, wl).x != -1.f;
        v = make_float2(fill0, fill1);
    }
    if (L.mode == 0) v.x = f_div(f_sub(v.x, L.mean), L.std);
    img[(size_t)w * H + h] = v.x;
    img[(size_t)W * H + (size_t)w * H + h] = v.y;
    mask[(size_t)w * H + h] = m;
    car[(size_t)w * H + h] = cw;
}

}  // namespace

// ---- handle -----------------------------------------------------------------------------------------------------
struct rldm_lidar {
    rldm_lidar_config cfg;
    float* tables = nullptr;                  // [4][H]: cos(incl), sin(incl), incl, height
    std::map<int, float*> azimuth;            // W -> [2][W]: cos(azi), sin(azi)
    int* chunk_counts = nullptr;
    size_t chunk_cap = 0;
    unsigned long long* keys = nullptr;       // projection scratch [H][W] + raw (H, W, 2)
    float2* raw = nullptr;
    size_t proj_cap = 0;
    void* ordered = nullptr;                  // rldm_lidar_to_voxel_ordered's scratch: keys, ids (both twice), votes, table, segments
    size_t ordered_cap = 0;                   // bytes
    LidarDev dev() const {
        LidarDev L;
        L.cos_incl = tables;
        L.sin_incl = tables + cfg.beams;
        L.incl = tables + 2 * cfg.beams;
        L.height = tables + 3 * cfg.beams;
        L.H = cfg.beams;
        L.mode = cfg.mode;
        L.mean = cfg.mean;
        L.std = cfg.std;
        L.range_fill = cfg.range_fill;
        L.intensity_fill = cfg.intensity_fill;
        return L;
    }
};

static int lidar_azimuth(rldm_lidar* l, int W, const float** cos_azi, const float** sin_azi) {
    auto it = l->azimuth.find(W);
    if (it == l->azimuth.end()) {
        // ldm/dataset.py:266-267 in fp32 steps like the torch expression, then cos / sin of that fp32 angle
        std::vector<float> t(2 * (size_t)W);
        const float pi_f = (float)M_PI;
        for (int w = 0; w < W; ++w) {
            volatile float a = ((float)W - 0.5f) - (float)w;
            a = a / (float)W;
            a = a * 2.f;
            a = a * pi_f;
            a = a - pi_f;
            t[w] = (float)cos((double)a);
            t[W + w] = (float)sin((double)a);
        }
        float* d = nullptr;
        RLDM_HIP_CHECK(hipMalloc(&d, t.size() * sizeof(float)));
        RLDM_HIP_CHECK(hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        it = l->azimuth.emplace(W, d).first;
    }
    *cos_azi = it->second;
    *sin_azi = it->second + W;
    return 0;
}

extern "C" {

int rldm_lidar_create(const rldm_lidar_config* cfg, const float* incl, const float* height, rldm_lidar** out) {
    RLDM_REQUIRE(cfg && incl && height && out, "null argument");
    RLDM_REQUIRE(cfg->beams > 0 && cfg->beams <= 4096, "beams out of range");
    RLDM_REQUIRE(cfg->mode >= 0 && cfg->mode <= 2, "mode must be 0 (linear), 1 (log) or 2 (inverse)");
    RLDM_REQUIRE(cfg->grid[0] > 0 && cfg->grid[1] > 0 && cfg->grid[2] > 0, "grid_sizes must be positive");
    auto* l = new rldm_lidar();
    l->cfg = *cfg;
    const int H = cfg->beams;
    std::vector<float> t(4 * (size_t)H);
    for (int h = 0; h < H; ++h) {
        t[h] = (float)cos((double)incl[h]);
        t[H + h] = (float)sin((double)incl[h]);
        t[2 * H + h] = incl[h];
        t[3 * H + h] = height[h];
    }
    if (hipMalloc(&l->tables, t.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(l->tables, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        rldm::set_error("rldm_lidar_create: device allocation failed");
        delete l;
        return 1;
    }
    *out = l;
    return 0;
}

void rldm_lidar_destroy(rldm_lidar* l) {
    if (!l) return;
    if (l->tables) (void)hipFree(l->tables);
    for (auto& kv : l->azimuth) (void)hipFree(kv.second);
    if (l->chunk_counts) (void)hipFree(l->chunk_counts);
    if (l->keys) (void)hipFree(l->keys);
    if (l->raw) (void)hipFree(l->raw);
    if (l->ordered) (void)hipFree(l->ordered);
    delete l;
}

int rldm_lidar_to_points(rldm_lidar* l, const float* range_images, int B, int C, int W, float* points, void* stream) {
    RLDM_REQUIRE(l && range_images && points, "null argument");
    RLDM_REQUIRE(B > 0 && C >= 1 && W > 0, "bad shape");
    const float *ca, *sa;
    if (lidar_azimuth(l, W, &ca, &sa)) return 1;
    const int N = W * l->cfg.beams;
    range_to_points_kernel<<<dim3((N + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(range_images, C, W, l->cfg.beams,
                                                                                    l->dev(), ca, sa, points);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_lidar_to_voxel(rldm_lidar* l, const float* range_images, int B, int C, int W, float* voxel, void* stream) {
    RLDM_REQUIRE(l && range_images && voxel, "null argument");
    RLDM_REQUIRE(B > 0 && W > 0, "bad shape");
    RLDM_REQUIRE(C >= 2, "to_voxel needs the remission channel (ldm/dataset.py:286 splats pc[:, :, 3:])");
    const float *ca, *sa;
    if (lidar_azimuth(l, W, &ca, &sa)) return 1;
    const rldm_lidar_config& c = l->cfg;
    GridDev G;
    G.gz = c.grid[0]; G.gy = c.grid[1]; G.gx = c.grid[2];
    // fp32 like the torch expressions (ldm/dataset.py:283-284)
    G.cx = (c.pc_range[3] + c.pc_range[0]) / 2.f; G.hx = (c.pc_range[3] - c.pc_range[0]) / 2.f;
    G.cy = (c.pc_range[4] + c.pc_range[1]) / 2.f; G.hy = (c.pc_range[4] - c.pc_range[1]) / 2.f;
    G.cz = (c.pc_range[5] + c.pc_range[2]) / 2.f; G.hz = (c.pc_range[5] - c.pc_range[2]) / 2.f;
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    hipStream_t st = (hipStream_t)stream;
    RLDM_HIP_CHECK(hipMemsetAsync(voxel, 0, (size_t)B * 2 * nvox * sizeof(float), st));
    const int N = W * c.beams;
    bev_splat_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(range_images, C, W, c.beams, l->dev(), ca, sa, G, voxel);
    RLDM_HIP_CHECK(hipGetLastError());
    bev_finalize_kernel<<<dim3((unsigned)((nvox + 255) / 256), B), 256, 0, st>>>(voxel, nvox, c.normalize_volume_densities, 1e-4f);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

static GridDev lidar_grid(const rldm_lidar_config& c) {
    GridDev G;
    G.gz = c.grid[0]; G.gy = c.grid[1]; G.gx = c.grid[2];
    G.cx = (c.pc_range[3] + c.pc_range[0]) / 2.f; G.hx = (c.pc_range[3] - c.pc_range[0]) / 2.f;
    G.cy = (c.pc_range[4] + c.pc_range[1]) / 2.f; G.hy = (c.pc_range[4] - c.pc_range[1]) / 2.f;
    G.cz = (c.pc_range[5] + c.pc_range[2]) / 2.f; G.hz = (c.pc_range[5] - c.pc_range[2]) / 2.f;
    return G;
}

int rldm_lidar_to_voxel_train(rldm_lidar* l, const float* range_images, int B, int C, int W, float* raw, float* voxel,
                              void* stream) {
    RLDM_REQUIRE(l && range_images && raw && voxel, "null argument");
    RLDM_REQUIRE(B > 0 && W > 0, "bad shape");
    RLDM_REQUIRE(C >= 2, "to_voxel needs the remission channel (ldm/dataset.py:286 splats pc[:, :, 3:])");
    const float *ca, *sa;
    if (lidar_azimuth(l, W, &ca, &sa)) return 1;
    const rldm_lidar_config& c = l->cfg;
    const GridDev G = lidar_grid(c);
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    hipStream_t st = (hipStream_t)stream;
    RLDM_HIP_CHECK(hipMemsetAsync(raw, 0, (size_t)B * 2 * nvox * sizeof(float), st));
    const int N = W * c.beams;
    bev_splat_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(range_images, C, W, c.beams, l->dev(), ca, sa, G, raw);
    RLDM_HIP_CHECK(hipGetLastError());
    bev_finalize_train_kernel<<<dim3((unsigned)((nvox + 255) / 256), B), 256, 0, st>>>(raw, voxel, nvox,
                                                                                     c.normalize_volume_densities, 1e-4f);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_lidar_to_voxel_ordered(rldm_lidar* l, const float* range_images, int B, int C, int W, float* raw, float* voxel,
                                void* stream) {
    RLDM_REQUIRE(l && range_images && raw && voxel, "null argument");
    RLDM_REQUIRE(B > 0 && W > 0, "bad shape");
    RLDM_REQUIRE(C >= 2, "to_voxel needs the remission channel (ldm/dataset.py:286 splats pc[:, :, 3:])");
    const rldm_lidar_config& c = l->cfg;
    const GridDev G = lidar_grid(c);
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    RLDM_REQUIRE(8ull * (unsigned long long)B * (unsigned long long)W * (unsigned long long)c.beams < (1ull << 31),
                 "to_voxel_ordered: 8 * B * W * beams votes must stay below 2^31");
    RLDM_REQUIRE(nvox < ((size_t)1 << 31), "to_voxel_ordered: the grid must have fewer than 2^31 cells");
    const float *ca, *sa;
    if (lidar_azimuth(l, W, &ca, &sa)) return 1;
    const int N = W * c.beams;
    const int M = 8 * N;                                        // votes per image
    const int nchunks = (M + ORD_CHUNK - 1) / ORD_CHUNK;
    int bits = 0;
    while (((size_t)1 << bits) < nvox + 1) ++bits;              // ceil(log2(nvox + 1)): the sentinel nvox is a key, too
    const int passes = (bits + 7) / 8;
    // scratch, every part rounded up to 256 bytes: keys and ids twice (the sort alternates), the votes, the digit table, the digit
    // totals, the segments
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t words = up((size_t)B * M * 4), votes = up((size_t)B * M * 8), table_b = up((size_t)B * 256 * nchunks * 4),
                 totals_b = up((size_t)B * 256 * 4), seg_b = up((size_t)B * nvox * 8);
    const size_t need = 4 * words + votes + table_b + totals_b + seg_b;
    if (need > l->ordered_cap) {
        if (l->ordered) RLDM_HIP_CHECK(hipFree(l->ordered));
        l->ordered = nullptr;
        l->ordered_cap = 0;
        RLDM_HIP_CHECK(hipMalloc(&l->ordered, need));
        l->ordered_cap = need;
    }
    char* p = static_cast<char*>(l->ordered);
    unsigned* keys[2] = {reinterpret_cast<unsigned*>(p), reinterpret_cast<unsigned*>(p + words)};
    int* ids[2] = {reinterpret_cast<int*>(p + 2 * words), reinterpret_cast<int*>(p + 3 * words)};
    float2* vals = reinterpret_cast<float2*>(p + 4 * words);
    int* table = reinterpret_cast<int*>(p + 4 * words + votes);
    int* totals = reinterpret_cast<int*>(p + 4 * words + votes + table_b);
    int2* seg = reinterpret_cast<int2*>(p + 4 * words + votes + table_b + totals_b);
    hipStream_t st = (hipStream_t)stream;
    bev_votes_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(range_images, C, W, c.beams, l->dev(), ca, sa, G, keys[0], vals);
    RLDM_HIP_CHECK(hipGetLastError());
    const dim3 sort_grid((nchunks + 3) / 4, B);
    int cur = 0;
    for (int pass = 0; pass < passes; ++pass, cur ^= 1) {
        radix_hist_kernel<<<sort_grid, 256, 0, st>>>(keys[cur], M, nchunks, 8 * pass, table);
        RLDM_HIP_CHECK(hipGetLastError());
        radix_scan_kernel<<<dim3(64, B), 256, 0, st>>>(table, nchunks, totals);
        RLDM_HIP_CHECK(hipGetLastError());
        radix_scatter_kernel<<<sort_grid, 256, 0, st>>>(keys[cur], pass ? ids[cur] : nullptr, M, nchunks, 8 * pass, table, totals,
                                                       keys[cur ^ 1], ids[cur ^ 1]);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    RLDM_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)B * nvox * sizeof(int2), st));
    bev_segments_kernel<<<dim3((M + 255) / 256, B), 256, 0, st>>>(keys[cur], M, (unsigned)nvox, seg);
    RLDM_HIP_CHECK(hipGetLastError());
    const dim3 cell_grid((unsigned)((nvox + 255) / 256), B);
    bev_ordered_sum_kernel<<<cell_grid, 256, 0, st>>>(seg, ids[cur], vals, M, (unsigned)nvox, raw);
    RLDM_HIP_CHECK(hipGetLastError());
    bev_finalize_train_kernel<<<cell_grid, 256, 0, st>>>(raw, voxel, nvox, c.normalize_volume_densities, 1e-4f);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_lidar_to_voxel_backward(rldm_lidar* l, const float* range_images, int B, int C, int W, const float* raw,
                                 const float* dvoxel, float* cell_grad, float* dimages, void* stream) {
    RLDM_REQUIRE(l && range_images && raw && dvoxel && cell_grad && dimages, "null argument");
    RLDM_REQUIRE(B > 0 && W > 0, "bad shape");
    RLDM_REQUIRE(C >= 2, "to_voxel needs the remission channel (ldm/dataset.py:286 splats pc[:, :, 3:])");
    const float *ca, *sa;
    if (lidar_azimuth(l, W, &ca, &sa)) return 1;
    const rldm_lidar_config& c = l->cfg;
    const GridDev G = lidar_grid(c);
    const size_t nvox = (size_t)G.gz * G.gy * G.gx;
    hipStream_t st = (hipStream_t)stream;
    bev_cell_grad_kernel<<<dim3((unsigned)((nvox + 255) / 256), B), 256, 0, st>>>(raw, dvoxel, cell_grad, nvox,
                                                                                c.normalize_volume_densities, 1e-4f);
    RLDM_HIP_CHECK(hipGetLastError());
    const int N = W * c.beams;
    bev_pixel_grad_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(range_images, C, W, c.beams, l->dev(), ca, sa, G, cell_grad,
                                                                    dimages);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_lidar_filter_points(rldm_lidar* l, const float* points, int B, int N, int cols, float max_depth, float* out,
                             int32_t* counts, void* stream) {
    RLDM_REQUIRE(l && points && out && counts, "null argument");
    RLDM_REQUIRE(B > 0 && N > 0 && (cols == 3 || cols == 4), "bad shape (cols must be 3 or 4)");
    const int nchunks = (N + 255) / 256;
    const size_t need = (size_t)B * nchunks;
    if (need > l->chunk_cap) {
        if (l->chunk_counts) RLDM_HIP_CHECK(hipFree(l->chunk_counts));
        l->chunk_counts = nullptr;
        RLDM_HIP_CHECK(hipMalloc(&l->chunk_counts, need * sizeof(int)));
        l->chunk_cap = need;
    }
    hipStream_t st = (hipStream_t)stream;
    filter_count_kernel<<<dim3(nchunks, B), 256, 0, st>>>(points, N, cols, max_depth, l->chunk_counts);
    RLDM_HIP_CHECK(hipGetLastError());
    filter_scatter_kernel<<<dim3(nchunks, B), 256, 0, st>>>(points, N, cols, max_depth, l->chunk_counts, out, counts);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_render_u8(const float* src, int B, int C, int W, int H, int channel, uint8_t* dst, void* stream) {
    RLDM_REQUIRE(src && dst, "null argument");
    RLDM_REQUIRE(B > 0 && C > 0 && W > 0 && H > 0 && channel >= 0 && channel < C, "bad shape");
    render_u8_kernel<<<dim3((W + 63) / 64, (H + 63) / 64, B), 256, 0, (hipStream_t)stream>>>(src, C, W, H, channel, dst);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int rldm_lidar_project(rldm_lidar* l, const float* points, int n_points, int stride, const int32_t* rows, float min_depth,
                       float* image, uint8_t* mask, uint8_t* car_window_mask, void* stream) {
    RLDM_REQUIRE(l && (points || n_points == 0) && image && mask && car_window_mask, "null argument");
    RLDM_REQUIRE(n_points >= 0 && stride >= 4, "points must carry at least x, y, z, intensity");
    const rldm_lidar_config& c = l->cfg;
    const int W = c.width, H = c.beams;
    RLDM_REQUIRE(W > 0, "config.width must be positive");
    const size_t px = (size_t)W * H;
    if (px > l->proj_cap) {
        if (l->keys) RLDM_HIP_CHECK(hipFree(l->keys));
        if (l->raw) RLDM_HIP_CHECK(hipFree(l->raw));
        l->keys = nullptr; l->raw = nullptr;
        RLDM_HIP_CHECK(hipMalloc(&l->keys, px * sizeof(unsigned long long)));
        RLDM_HIP_CHECK(hipMalloc(&l->raw, px * sizeof(float2)));
        l->proj_cap = px;
    }
    hipStream_t st = (hipStream_t)stream;
    RLDM_HIP_CHECK(hipMemsetAsync(l->keys, 0xff, px * sizeof(unsigned long long), st));
    const LidarDev L = l->dev();
    if (n_points > 0) {
        project_keys_kernel<<<(n_points + 255) / 256, 256, 0, st>>>(points, n_points, stride, rows, L, W, min_depth, l->keys);
        RLDM_HIP_CHECK(hipGetLastError());
    }
    project_gather_kernel<<<(unsigned)((px + 255) / 256), 256, 0, st>>>(l->keys, points, stride, L, W, l->raw);
    RLDM_HIP_CHECK(hipGetLastError());
    // ldm/dataset.py:212-217: what a still-missing pixel is filled with
    float fill0 = c.range_fill, fill1 = c.intensity_fill;
    if (c.mode == 1) { fill0 = (float)(log2((double)c.range_fill + 1.0) / 6.0); fill1 = (float)(log2((double)c.intensity_fill + 1.0) / 6.0); }
    else if (c.mode == 2) fill0 = (float)(1.0 / (double)c.range_fill);
    project_finish_kernel<<<(unsigned)((px + 255) / 256), 256, 0, st>>>(l->raw, L, W, fill0, fill1, image, mask, car_window_mask);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
