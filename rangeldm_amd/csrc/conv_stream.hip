// Weight-streaming circular 3x3 convolution for the full-resolution levels (UNet 256x16, VAE decoder) on gfx950:
// bf16 MFMA 32x32x16, fp32 accumulate, 256 pixels x 128 channels per workgroup.
//
// Same fused unit as conv_igemm.hip -- GroupNorm + SiLU of cat[x0, x1] on the way into LDS, conv 3x3 (wrap W / zero H,
// optional nearest-x2 folded into the indexing), bias + time embedding, shortcut-conv / residual as extra K over the raw
// block input, per-channel statistics of the output for the next GroupNorm (ldm/utils.py:40-58,107-116;
// vae/sgm/modules/diffusionmodules/model.py:93-125,342-362) -- with a different division of labour between LDS and L2:
//   * only the ACTIVATIONS go through LDS: per 64-channel chunk the halo of the 32x8 pixel tile (34x10 positions) is
//     double-buffered, chunk c+1 is fetched and normalised while chunk c computes, and the workgroup meets at ONE barrier
//     per chunk (conv_igemm.hip: one per tap, because its weight ring lives in LDS too);
//   * the WEIGHTS are packed on the host in MFMA A-fragment order, one contiguous stream of 1 KiB k-steps per 32-channel
//     tile, and every wave loads its own fragments straight from L2 into registers: a ring of 12 fragments (one row of
//     taps) in flight, refilled in program order so the compiler's s_waitcnt counts are exact; the stream never stops at
//     a barrier;
//   * 8 waves = 2 pixel halves x 4 channel tiles; a wave owns 128 pixels x 32 channels (4 MFMAs per fragment), so each
//     fragment is requested by two waves (the second hit is an L1 hit) and the LDS feeds 4 pixel fragments per k-step;
//   * waves 0-3 normalise their share of the next chunk after the first row of taps, waves 4-7 after the second, so the
//     VALU work (GroupNorm affine + SiLU) of one half runs under the other half's MFMAs: the two waves of a SIMD are never
//     both in it.
// Second instance for the 128x8 level (too few 256-pixel tiles to fill the chip): 128 pixels x 64 channels per workgroup,
// 8 waves = 2 channel tiles x 4 k-groups (k-group kg owns the kg-th 16-channel group of every tap of a chunk: one k-step
// per tap, ring = the 9 steps of a chunk); the k-groups' fp32 partial tiles meet in LDS for the epilogue (conv_small.hip's).
#include "conv_stream_body.h"
#include "conv_stream_spec_body.h"

#include <utility>

namespace rldm {

// WM pixel parts (128 pixels each) x WN 32-channel tiles x KG k-groups = NW waves; the 4-wave instances are built for two workgroups
// per CU (__launch_bounds__' second argument is waves per SIMD: 2 x 256 threads = 2).  Instantiated from the rows of kStreamInst (kernels.h)
template <int WM, int WN, int NW, int MI, int S, bool SUB, bool T4, bool FH>
__global__ void __launch_bounds__((StreamInstDesc{WM, WN, NW, MI}.threads()), (StreamInstDesc{WM, WN, NW, MI}.wg_per_cu())) conv_stream_kernel(const ConvParams p) {
    // Workgroups are dispatched x-fastest and land on XCD (linear id % 8).  Re-number them so that every XCD owns a contiguous
    // run of (image, pixel tile, channel tile) ids: the tiles of an image then share ONE L2, and the halo rows two neighbouring
    // tiles both read (34 x 10 positions for 32 x 8 pixels: 1.33x the tile) are fetched from HBM / Infinity Cache once.
    int nt, mt, b;
    {
        const int gx = p.ntile_n, gy = p.tiles_img;    // (== gridDim.x / .y: from the arguments, not a dependent read of the dispatch packet)
        const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const int rid = (p.dbg & (1 << 21)) ? lin : xcd_remap(lin, gx * gy * p.B);
        const int q = rid / gx;
        nt = rid - q * gx;
        b = q / gy;
        mt = q - b * gy;
    }
    const TrunkSeam none = {};
    conv_stream_body<WM, WN, false, NW, MI, S, SUB, T4, FH>(p, nt, mt, b, none);
}

// the 256 x 128 tile with specialised waves (conv_stream_spec_body.h): 4 matrix waves + 4 staging waves
__global__ void __launch_bounds__(512, 1) conv_stream_spec_kernel(const ConvParams p) {
    int nt, mt, b;
    {
        const int gx = p.ntile_n, gy = p.tiles_img;
        const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const int rid = (p.dbg & (1 << 21)) ? lin : xcd_remap(lin, gx * gy * p.B);
        const int q = rid / gx;
        nt = rid - q * gx;
        b = q / gy;
        mt = q - b * gy;
    }
    const TrunkSeam none = {};
    conv_stream_spec_body<false>(p, nt, mt, b, none);
}

// ---------------------------------------------------------------------------------------------------------------
// host side: every figure of an instance is read from its row of kStreamInst (kernels.h)
// ---------------------------------------------------------------------------------------------------------------
int conv_stream_bn(const ConvParams& p) { return stream_inst(p).bn(); }
int conv_stream_kgroups(const ConvParams& p) { return stream_inst(p).kgroups(); }
int conv_stream_threads(const ConvParams& p) { return stream_inst(p).threads(); }

size_t conv_stream_lds_bytes(const ConvParams& p) {
    const int BN = conv_stream_bn(p), KG = conv_stream_kgroups(p), BM = p.TW * p.TH;
    const size_t a = (size_t)((p.TW - 1) * p.stride + 3) * p.colb;
    const size_t main_bytes = 2 * a + (size_t)(p.C0 + p.C1) * 8 + BN * 4;
    const size_t gscratch = p.st0 ? (size_t)2 * (p.C0 + p.C1) * 8 : 0;
    const size_t epi = KG == 1 ? (size_t)BM * (BN * 2 + 16) + (size_t)8 * 2 * BN * 4
                               : (size_t)KG * 64 * (BN * 4 + 16) + (size_t)64 * (BN * 2 + 16) + (size_t)8 * 2 * BN * 4;
    return std::max(std::max(main_bytes, gscratch), epi);
}

bool conv_stream_supported(const ConvParams& p, int taps) {
    if (p.st_inst < 0 || p.st_inst >= SI_COUNT) return false;
    const StreamInstDesc& d = stream_inst(p);
    const int Cin = p.C0 + p.C1, R = p.R0 + p.R1;
    // common to all instances
    if (taps != 9 || p.pad_lo != 1 || (p.up != 1 && p.up != 2) || p.y_nchw || p.ksplit > 1) return false;
    if (Cin % 64 != 0 || (p.C1 != 0 && p.C0 % 64 != 0) || R % 64 != 0 || (p.R1 != 0 && p.R0 % 64 != 0)) return false;
    if (R != 0 && p.up != 1) return false;
    if (p.Win * p.up < 2 || p.N % d.bn() != 0 || Cin > 512) return false;
    if (p.st0 && (p.gn_groups > 64 || Cin % p.gn_groups != 0)) return false;
    if ((p.tiles_h & (p.tiles_h - 1)) != 0 || p.B > 65535 || p.tiles_img > 65535) return false;
    // the instance's own
    if (p.stride != d.STR || !d.takes(p.TW, p.TH) || (d.up1 && p.up != 1) || (d.no_res && R != 0)) return false;
    if (d.SUB && (p.Wout != 2 * p.Win || p.Hout != 2 * p.Hin)) return false;     // (tiles over the INPUT, four parities per tile)
    if (d.FH && p.Hout != p.TH) return false;
    return conv_stream_lds_bytes(p) <= (size_t)d.lds_cap();
}

// one launcher -- and one DynLdsLimit (per device, thread safe) -- per row of the table, i.e. per kernel (conv_regw.hip: why not a shared one)
template <int I>
static int launch_stream_inst(const ConvParams& p, size_t lds, hipStream_t stream) {
    constexpr StreamInstDesc d = kStreamInst[I];
    void (*kern)(const ConvParams);
    if constexpr (d.spec) kern = conv_stream_spec_kernel;
    else kern = conv_stream_kernel<d.WM, d.WN, d.NW, d.MI, d.STR, d.SUB, d.T4, d.FH>;
    static DynLdsLimit lds_limit;
    RLDM_HIP_CHECK(lds_limit.ensure(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(p.N / d.bn() * (d.SUB ? 4 : 1), p.tiles_img, p.B), dim3(d.threads()), lds, stream, p);
    RLDM_HIP_CHECK(hipGetLastError());
    return 0;
}
template <int... I>
static int launch_stream_row(const ConvParams& p, size_t lds, hipStream_t stream, std::integer_sequence<int, I...>) {
    static constexpr int (*launch[])(const ConvParams&, size_t, hipStream_t) = {launch_stream_inst<I>...};
    return launch[p.st_inst](p, lds, stream);
}

int launch_conv_stream(const ConvParams& p, hipStream_t stream) {
    RLDM_REQUIRE(conv_stream_supported(p, 9), "conv_stream: unsupported shape");
    return launch_stream_row(p, conv_stream_lds_bytes(p), stream, std::make_integer_sequence<int, SI_COUNT>());
}

}  // namespace rldm
