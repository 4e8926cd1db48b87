// Host parameters and the device images the kernels read them from: the parameter store, the ConvLayer packers (one weight layout
// per kernel family), the per-head attention fragments.
#include "runtime.h"

namespace rldm {

// conv_igemm.hip image: [ntile_n][Cin_pad/CK * taps + R/CK][BN][CK + 8] bf16; channel rows >= Cout and channels >= Cin are
// zero; bias padded to ntile_n * BN
int ConvLayer::get_packed(int BN, int CK, int Cin_pad, Packed** out) {
    return cached({WeightLayout::Igemm, BN, CK}, Cin_pad, out, [&](std::vector<bf16_t>& img, std::vector<float>& bias) {
        RLDM_REQUIRE(R % CK == 0, "conv " + name + ": residual channels not a multiple of the channel chunk");
        const int taps = ksize * ksize;
        const int ntile = (Cout + BN - 1) / BN;
        const int ncc = Cin_pad / CK, ncb = R / CK;
        const int RSE = CK + 8;
        const size_t stages = (size_t)ncc * taps + ncb;
        img.assign((size_t)ntile * stages * BN * RSE, 0);
        auto at = [&](int n, size_t stage, int ck) -> bf16_t& { return img[(((size_t)(n / BN) * stages + stage) * BN + n % BN) * RSE + ck]; };
        for (int n = 0; n < Cout; ++n) {
            for (int c = 0; c < Cin; ++c)
                for (int tap = 0; tap < taps; ++tap) at(n, (size_t)(c / CK) * taps + tap, c % CK) = f32_to_bf16(weight(n, c, tap));
            for (int c = 0; c < R; ++c) at(n, (size_t)ncc * taps + c / CK, c % CK) = f32_to_bf16(res_weight(n, c));
        }
        bias.resize((size_t)ntile * BN, 0.f);
        return 0;
    });
}

// conv_stream.hip image: MFMA A-fragment order, one contiguous stream of 1 KiB k-steps per (32-channel tile, k-group):
// [Cout/32][KG][Cin_pad/64 chunks x 9 taps x 4/KG k-steps, then R/64 chunks x 4/KG k-steps][64 lanes][8 bf16] + 32 KiB
// of zeros (the ring's read-ahead past the last stream: up to 18 fragments of 1 KiB in the 64-pixel instance); k-group kg owns the k-steps [kg*4/KG, (kg+1)*4/KG) of every
// tap of a chunk; lane l holds channel 32*t + (l & 31), k = 8*(l >> 5) .. +8 of the step; bias padded to whole tiles
int ConvLayer::get_streampacked(int Cin_pad, int KG, Packed** out) {
    return cached({WeightLayout::Stream, KG, 0}, Cin_pad, out, [&](std::vector<bf16_t>& img, std::vector<float>& bias) {
        RLDM_REQUIRE(ksize == 3 && (Cout % 32 == 0 || Cout < 32) && Cin_pad % 64 == 0 && R % 64 == 0, "conv " + name + ": not stream-packable");
        const int SPT = 4 / KG, NCC = Cin_pad / 64, NCB = R / 64, nsteps = (NCC * 9 + NCB) * SPT;
        const int ntile32 = (Cout + 31) / 32;        // (fewer than 32 output channels -- conv_regw.hip's conv_out: one tile, zero rows and zero bias behind them)
        img.assign((size_t)ntile32 * KG * nsteps * 512 + 16384, 0);
        auto at = [&](int n, int ks, int step, int k) -> bf16_t& {      // ks: 16-channel group within the 64-channel chunk
            const size_t stream = (size_t)(n / 32) * KG + ks / SPT;
            return img[((stream * nsteps + step + ks % SPT) * 64 + (k / 8) * 32 + n % 32) * 8 + k % 8];
        };
        for (int n = 0; n < Cout; ++n) {
            for (int c = 0; c < Cin; ++c)
                for (int tap = 0; tap < 9; ++tap) at(n, (c % 64) / 16, ((c / 64) * 9 + tap) * SPT, c % 16) = f32_to_bf16(weight(n, c, tap));
            for (int c = 0; c < R; ++c) at(n, (c % 64) / 16, (NCC * 9 + c / 64) * SPT, c % 16) = f32_to_bf16(res_weight(n, c));
        }
        bias.resize((size_t)ntile32 * 32, 0.f);
        return 0;
    });
}

// conv_regw.hip, conv_c16_kernel (the input layer: <= 16 input channels): [Cout / 32][9 taps][64 lanes][8 bf16] -- lane l of a fragment holds
// channel 32 t + (l & 31), input channels 8 (l >> 5) .. + 8
int ConvLayer::get_c16packed(Packed** out) {
    return cached({WeightLayout::C16, 0, 0}, 16, out, [&](std::vector<bf16_t>& img, std::vector<float>&) {
        RLDM_REQUIRE(ksize == 3 && Cout % 32 == 0 && Cin <= 16 && R == 0, "conv " + name + ": not a 16-channel input layer");
        img.assign((size_t)(Cout / 32) * 9 * 512, 0);
        for (int n = 0; n < Cout; ++n)
            for (int c = 0; c < Cin; ++c)
                for (int tap = 0; tap < 9; ++tap)
                    img[(((size_t)(n / 32) * 9 + tap) * 64 + (c / 8) * 32 + n % 32) * 8 + c % 8] = f32_to_bf16(weight(n, c, tap));
        return 0;
    });
}

// conv_stream.hip, sub-pixel form of nearest x2 + 3x3 (conv_stream_body.h, SUB): per (32-channel tile, parity pw * 2 + ph) one stream
// [Cin_pad/64 chunks][2 x 2 taps (w-major)][4 k-steps][64 lanes][8 bf16] of SUMMED weights -- along each axis parity 0 reads inputs
// (x - 1, x) through (k[0], k[1] + k[2]), parity 1 reads (x, x + 1) through (k[0] + k[1], k[2]); summed in fp32, rounded once
int ConvLayer::get_subpixpacked(int Cin_pad, Packed** out) {
    return cached({WeightLayout::SubPixel, 0, 0}, Cin_pad, out, [&](std::vector<bf16_t>& img, std::vector<float>&) {
        RLDM_REQUIRE(ksize == 3 && Cout % 32 == 0 && Cin_pad % 64 == 0 && R == 0, "conv " + name + ": not sub-pixel-packable");
        const int NCC = Cin_pad / 64, nsteps = NCC * 16;
        img.assign((size_t)(Cout / 32) * 4 * nsteps * 512 + 16384, 0);
        static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};    // [parity][tap]: original taps lo .. hi summed
        for (int n = 0; n < Cout; ++n)
            for (int c = 0; c < Cin; ++c)
                for (int pw = 0; pw < 2; ++pw)
                    for (int ph = 0; ph < 2; ++ph)
                        for (int i = 0; i < 2; ++i)
                            for (int j = 0; j < 2; ++j) {
                                float v = 0.f;
                                for (int a = lo[pw][i]; a <= hi[pw][i]; ++a)
                                    for (int bb = lo[ph][j]; bb <= hi[ph][j]; ++bb) v += weight(n, c, a * 3 + bb);
                                const size_t stream = (size_t)(n / 32) * 4 + pw * 2 + ph;
                                const int step = ((c / 64) * 4 + i * 2 + j) * 4 + (c % 64) / 16, k = c % 16;
                                img[((stream * nsteps + step) * 64 + (k / 8) * 32 + n % 32) * 8 + k % 8] = f32_to_bf16(v);
                            }
        return 0;
    });
}

// conv_small.hip image: MFMA A-fragment order, one contiguous stream of 1 KiB k-steps per (TN-channel tile, k-group):
// [Cout/TN][KG][taps*CPT main steps (tap-major) + RPT residual steps][64 lanes][8 bf16] + one zero fragment.  A k-step is
// 512 / TN input channels of a tap; k-group kg owns the channel groups kg, kg + KG, ... of every tap.
// TN == 32: k-steps of 16 channels, lane l holds channel 32*t + (l & 31), k = 8*(l >> 5) .. +8;
// TN == 16 (the image-owning 16-channel tiles, KG == 8): k-steps of 32 channels (v_mfma_f32_16x16x32_bf16), lane l holds
// channel 16*t + (l & 15), k = 8*(l >> 4) .. +8.
// `no_res`: the (identity) residual is added by the kernel's epilogue, not multiplied here.
int ConvLayer::get_fragpacked(int Cin_pad, int TN, int KG, bool no_res, Packed** out) {
    const WeightLayout layout = no_res ? WeightLayout::FragNoRes : WeightLayout::Frag;
    return cached({layout, TN, KG}, Cin_pad, out, [&](std::vector<bf16_t>& img, std::vector<float>&) {
        const int taps = ksize * ksize, Rp = no_res ? 0 : R, KS = 512 / TN;
        RLDM_REQUIRE((TN == 32 || TN == 16) && Cout % TN == 0 && Cin_pad % (KS * KG) == 0 && Rp % (KS * KG) == 0,
                     "conv " + name + ": not fragment-packable");
        const int CPT = Cin_pad / KS / KG, RPT = Rp / KS / KG, nmine = taps * CPT + RPT;
        img.assign((size_t)(Cout / TN) * KG * nmine * 512 + 512, 0);
        auto at = [&](int n, int step0, int c) -> bf16_t& {             // step0: first step of the tap / of the residual phase
            const int cg = c / KS, k = c % KS;                          // channel group (k-group cg % KG, its step cg / KG), k within it
            const size_t stream = (size_t)(n / TN) * KG + cg % KG;
            return img[((stream * nmine + step0 + cg / KG) * 64 + (k / 8) * TN + n % TN) * 8 + k % 8];
        };
        for (int n = 0; n < Cout; ++n) {
            for (int c = 0; c < Cin; ++c)
                for (int tap = 0; tap < taps; ++tap) at(n, tap * CPT, c) = f32_to_bf16(weight(n, c, tap));
            for (int c = 0; c < Rp; ++c) at(n, taps * CPT, c) = f32_to_bf16(res_weight(n, c));
        }
        return 0;
    });
}

int ParamStore::set(const char* name, const float* data, int64_t numel) {
    auto it = expected.find(name);
    RLDM_REQUIRE(it != expected.end(), std::string("unexpected parameter key: ") + name);
    RLDM_REQUIRE(it->second == numel, std::string("size mismatch for ") + name + ": expected " +
                                          std::to_string(it->second) + " got " + std::to_string(numel));
    host[name].assign(data, data + numel);
    finalized = false;
    return 0;
}
int ParamStore::check_complete() const {
    for (auto& kv : expected)
        RLDM_REQUIRE(host.count(kv.first), std::string("missing parameter key: ") + kv.first);
    return 0;
}
void ParamStore::expect_conv(const std::string& n, int co, int ci, int k) {
    expected[n + ".weight"] = (int64_t)co * ci * k * k;
    expected[n + ".bias"] = co;
}
void ParamStore::expect_lin(const std::string& n, int co, int ci) {
    expected[n + ".weight"] = (int64_t)co * ci;
    expected[n + ".bias"] = co;
}
void ParamStore::expect_norm(const std::string& n, int c) {
    expected[n + ".weight"] = c;
    expected[n + ".bias"] = c;
}
void ParamStore::expect_resnet(const std::string& p, int ci, int co, int temb) {
    expect_norm(p + ".norm1", ci);
    expect_conv(p + ".conv1", co, ci, 3);
    if (temb) expect_lin(p + ".time_emb_proj", co, temb);
    expect_norm(p + ".norm2", co);
    expect_conv(p + ".conv2", co, co, 3);
    if (ci != co) expect_conv(p + ".conv_shortcut", co, ci, 1);
}
void ParamStore::expect_attn(const std::string& p, int c) {
    expect_norm(p + ".group_norm", c);
    expect_lin(p + ".to_q", c, c);
    expect_lin(p + ".to_k", c, c);
    expect_lin(p + ".to_v", c, c);
    expect_lin(p + ".to_out.0", c, c);
}

int Layers::add_conv(ParamStore& ps, const std::string& n, int co, int ci, int k) {
    auto L = std::make_unique<ConvLayer>();
    L->name = n;
    L->Cout = co;
    L->Cin = ci;
    L->ksize = k;
    L->w = ps.host.at(n + ".weight");
    L->b = ps.host.at(n + ".bias");
    conv[n] = std::move(L);
    return 0;
}
int Layers::add_norm(ParamStore& ps, const std::string& n, int c) {
    auto N = std::make_unique<NormParams>();
    N->C = c;
    if (upload(N->gamma, ps.host.at(n + ".weight").data(), c * sizeof(float))) return 1;
    if (upload(N->beta, ps.host.at(n + ".bias").data(), c * sizeof(float))) return 1;
    norm[n] = std::move(N);
    return 0;
}
// fused q|k|v projection; q rows pre-scaled by log2(e)/sqrt(head_dim) so attention works in exp2 units
int Layers::add_qkv(ParamStore& ps, const std::string& p, int c, int head_dim) {
    auto L = std::make_unique<ConvLayer>();
    L->name = p + ".qkv";
    L->Cout = 3 * c;
    L->Cin = c;
    L->ksize = 1;
    const float qs = attn_q_scale(head_dim);
    const char* names[3] = {".to_q", ".to_k", ".to_v"};
    for (int i = 0; i < 3; ++i) {
        const auto& w = ps.host.at(p + names[i] + ".weight");
        const auto& b = ps.host.at(p + names[i] + ".bias");
        const float s = i == 0 ? qs : 1.f;
        for (float v : w) L->w.push_back(v * s);
        for (float v : b) L->b.push_back(v * s);
    }
    conv[L->name] = std::move(L);
    return 0;
}

// Per-head MFMA A fragments of the merged q|k|v Linear for attention_qkv_d8_kernel: w [3C][C] (q rows already scaled by
// log2(e)/sqrt(8)), b [3C] -> img [heads][C/16][64 lanes][8] bf16 (row = lane & 31: 0-7 q, 8-15 k, 16-23 v, 24-31 zero;
// channels 16*ks + 8*(lane >> 5) ..+8), bias [heads][32].
void pack_attn_head_frags(const float* w, const float* b, int C, std::vector<bf16_t>& img, std::vector<float>& bias) {
    const int heads = C / 8, nks = C / 16;
    img.assign((size_t)heads * nks * 512, 0);
    bias.assign((size_t)heads * 32, 0.f);
    for (int h = 0; h < heads; ++h)
        for (int row = 0; row < 24; ++row) {
            const int src = (row / 8) * C + h * 8 + row % 8;            // q | k | v rows of the merged Linear
            bias[(size_t)h * 32 + row] = b[src];
            for (int c = 0; c < C; ++c)
                img[(((size_t)h * nks + c / 16) * 64 + ((c % 16) / 8) * 32 + row) * 8 + c % 8] = f32_to_bf16(w[(size_t)src * C + c]);
        }
}

}  // namespace rldm
