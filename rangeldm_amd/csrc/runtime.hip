// librangeldm_hip runtime: the model objects (UNet2DModel, VAE), the network walks that turn them into execution plans (plan.hip:
// one activation arena + an ordered list of kernel launches) and their part of the C ABI of include/rangeldm_hip.h.  The weights
// live in weights.hip, the HIP-graph captured sampling loop in sampler.hip, the kernel-level test entry points in test_entry.hip.
//
// Network structure follows diffusers UNet2DModel.forward [3P; SURVEY.md A.2] as configured by
// ldm/train_unconditional.py:237-242 and the sgm Encoder/Decoder forward
// (vae/sgm/modules/diffusionmodules/model.py:852-896,1024-1057); the loop follows ldm/pipelines.py:353-367.
#include "runtime.h"

namespace rldm {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

// ---------------------------------------------------------------------------------------------------------------
// shared network pieces
// ---------------------------------------------------------------------------------------------------------------
struct NetCommon {
    Layers layers;
    int groups = 32;
    float eps = 1e-5f;
    int temb_ld = 0;                                 // total projected channels (0: no time embedding)
    std::map<std::string, int> temb_off;             // resnet prefix -> channel offset in the temb row

    // ---- a concatenation wider than the low-resolution conv kernel takes (RangeDM's 512-channel levels: 512 + 512 and 512 + 256
    // input channels, ldm/configs/RangeDM.yaml:19-21) -----------------------------------------------------------------------
    // conv_small.hip copies ALL input channels of its pixel tile to LDS (<= 512); past that the generic kernel walked K = 9216 on a
    // handful of workgroups (54-63 us per conv, 36 % of a RangeDM step at 0.9 % of the MFMA peak).  The convolution is linear in
    // its input channels, so the block runs as
    //     (a0, a1) = silu(GN1(cat[x, skip]))            one gn_apply launch, two output tensors (x.C | skip.C channels)
    //     t  = conv1[:, :x.C](a0)                       no bias
    //     h1 = conv1[:, x.C:](a1) + b1 + temb + t       t enters as the epilogue's identity residual
    //     u  = conv2(silu(GN2(h1))) + shortcut[:, :x.C](x) + b2 + b_sc       (the K-phase residual over x alone)
    //     y  = shortcut[:, x.C:](skip) + u              a 1x1 conv with u as its identity residual
    // -- four launches of the fast kernel for two of the slow one; t and u are rounded to bf16 on the way (one more rounding of a
    // partial sum: inside the network tolerance, tests/test_hip_models.py::test_other_presets_full_size_match_reference).
    // RLDM_FLAG_NO_WIDE_SPLIT keeps the two generic launches.
    bool wide_concat(const Builder& b, const Tensor& x, const Tensor& skip) const {
        if (dbg() & RLDM_FLAG_NO_WIDE_SPLIT) return false;
        if (!skip.valid() || x.C + skip.C <= 512 || x.C > 512 || skip.C > 512 || x.C % 64 != 0 || skip.C % 64 != 0) return false;
        const long long px = (long long)x.W * x.H;
        (void)b;
        return (px <= 256 || (long long)x.B * px <= 4096) && x.H >= 2;      // where conv_small.hip would run the halves
    }
    ConvLayer* derived_conv(const std::string& name, const ConvLayer* src, int c_lo, int c_hi, bool keep_bias) {
        if (ConvLayer* L = layers.get_conv(name)) return L;
        auto L = std::make_unique<ConvLayer>();
        const int taps = src->ksize * src->ksize, Ci = c_hi - c_lo;
        L->name = name;
        L->Cout = src->Cout; L->Cin = Ci; L->ksize = src->ksize;
        L->w.resize((size_t)src->Cout * Ci * taps);
        for (int n = 0; n < src->Cout; ++n)
            for (int c = 0; c < Ci; ++c)
                for (int t = 0; t < taps; ++t)
                    L->w[((size_t)n * Ci + c) * taps + t] = src->w[((size_t)n * src->Cin + c_lo + c) * taps + t];
        L->b = keep_bias ? src->b : std::vector<float>(src->Cout, 0.f);
        ConvLayer* raw = L.get();
        layers.conv[name] = std::move(L);
        return raw;
    }
    int resnet_wide(Builder& b, const std::string& p, Tensor x, Tensor skip, Tensor* out) {
        ConvLayer* c1 = layers.get_conv(p + ".conv1");
        ConvLayer* c2 = layers.get_conv(p + ".conv2");
        NormParams* n1 = layers.get_norm(p + ".norm1");
        const int Ctot = x.C + skip.C;
        RLDM_REQUIRE(c1 && c2 && n1 && c1->Cin == Ctot && c2->R == Ctot && !c2->sc_identity, "resnet " + p + ": not a wide concatenation");
        // -- GroupNorm + SiLU of the concatenation, once, into the two halves
        Tensor a0 = b.make(x.B, x.W, x.H, x.C), a1 = b.make(x.B, x.W, x.H, skip.C);
        RLDM_REQUIRE(x.P > 0 && skip.P > 0 && Ctot % groups == 0, "resnet " + p + ": GroupNorm input without statistics");
        b.note_launch();
        if (!b.dry) {
            GnApplyParams g;
            memset(&g, 0, sizeof(g));
            g.x0 = b.tptr(x); g.x1 = b.tptr(skip);
            g.C0 = x.C; g.C1 = skip.C;
            g.st0 = b.sptr(x); g.st1 = b.sptr(skip);
            g.P0 = x.P; g.P1 = skip.P;
            g.B = x.B; g.npix = x.W * x.H;
            g.groups = groups;
            g.gamma = n1->gamma.as<float>(); g.beta = n1->beta.as<float>();
            g.eps = eps; g.silu = 1;
            g.y = b.tptr(a0); g.y1 = b.tptr(a1); g.ysplit = x.C;
            b.plan->ops.push_back({[g](hipStream_t s) { return launch_gn_apply(g, s); }, "gn_apply_kernel", 0.0,
                                   (double)g.B * g.npix * Ctot * 4.0});
        }
        // -- conv1 in two halves
        ConvLayer* c1a = derived_conv(p + ".conv1@lo", c1, 0, x.C, false);
        ConvLayer* c1b = derived_conv(p + ".conv1@hi", c1, x.C, Ctot, true);
        c1b->R = c1b->Cout;
        c1b->sc_identity = true;
        ConvArgs A;
        A.layer = c1a; A.x0 = a0;
        Tensor t;
        if (b.conv(A, &t)) return 1;
        b.release(a0);
        ConvArgs B_;
        B_.layer = c1b; B_.x0 = a1; B_.r0 = t;
        auto it = temb_off.find(p);
        B_.temb_off = it == temb_off.end() ? -1 : it->second;
        B_.want_stats = true;
        Tensor h1;
        if (b.conv(B_, &h1)) return 1;
        b.release(a1);
        b.release(t);
        // -- conv2 with the shortcut over x in its K loop, then the shortcut over skip as a pointwise conv on top
        ConvLayer* c2a = layers.get_conv(p + ".conv2@lo");
        if (!c2a) {
            auto L = std::make_unique<ConvLayer>();         // (own host weights; the packed images are built per layer)
            L->name = p + ".conv2@lo";
            L->Cout = c2->Cout; L->Cin = c2->Cin; L->ksize = c2->ksize;
            L->w = c2->w;
            L->b = c2->b;
            L->R = x.C;
            L->sc_w.resize((size_t)c2->Cout * x.C);
            for (int n = 0; n < c2->Cout; ++n)
                for (int c = 0; c < x.C; ++c) L->sc_w[(size_t)n * x.C + c] = c2->sc_w[(size_t)n * Ctot + c];
            c2a = L.get();
            layers.conv[L->name] = std::move(L);
        }
        ConvLayer* c2b = layers.get_conv(p + ".conv2@hi");
        if (!c2b) {
            auto L = std::make_unique<ConvLayer>();
            L->name = p + ".conv2@hi";
            L->Cout = c2->Cout; L->Cin = skip.C; L->ksize = 1;
            L->w.resize((size_t)c2->Cout * skip.C);
            for (int n = 0; n < c2->Cout; ++n)
                for (int c = 0; c < skip.C; ++c) L->w[(size_t)n * skip.C + c] = c2->sc_w[(size_t)n * Ctot + x.C + c];
            L->b.assign(c2->Cout, 0.f);
            L->R = c2->Cout;
            L->sc_identity = true;
            c2b = L.get();
            layers.conv[L->name] = std::move(L);
        }
        ConvArgs C2;
        C2.layer = c2a; C2.x0 = h1;
        C2.gn = layers.get_norm(p + ".norm2");
        C2.eps = eps; C2.groups = groups; C2.silu = 1;
        C2.r0 = x;
        Tensor u;
        if (!Builder::small_route(C2, conv_shape(C2))) {
            // the 3x3 tile and the shortcut's input tile do not fit the LDS together (64x4 images: 112 + 67 KB): the shortcut over x
            // becomes a pointwise conv of its own as well --  u0 = conv2(..) + b;  u = shortcut[:, :x.C](x) + u0
            ConvLayer* c2m = layers.get_conv(p + ".conv2@main");
            if (!c2m) {
                auto L = std::make_unique<ConvLayer>();
                L->name = p + ".conv2@main";
                L->Cout = c2->Cout; L->Cin = c2->Cin; L->ksize = c2->ksize;
                L->w = c2->w;
                L->b = c2->b;
                c2m = L.get();
                layers.conv[L->name] = std::move(L);
            }
            ConvLayer* c2x = layers.get_conv(p + ".conv2@x");
            if (!c2x) {
                auto L = std::make_unique<ConvLayer>();
                L->name = p + ".conv2@x";
                L->Cout = c2->Cout; L->Cin = x.C; L->ksize = 1;
                L->w = c2a->sc_w;
                L->b.assign(c2->Cout, 0.f);
                L->R = c2->Cout;
                L->sc_identity = true;
                c2x = L.get();
                layers.conv[L->name] = std::move(L);
            }
            C2.layer = c2m;
            C2.r0 = Tensor();
            Tensor u0;
            if (b.conv(C2, &u0)) return 1;
            ConvArgs X;
            X.layer = c2x; X.x0 = x; X.r0 = u0;
            if (b.conv(X, &u)) return 1;
            b.release(u0);
        } else if (b.conv(C2, &u)) {
            return 1;
        }
        b.release(h1);
        ConvArgs D;
        D.layer = c2b; D.x0 = skip; D.r0 = u;
        D.want_stats = true;
        if (b.conv(D, out)) return 1;
        b.release(u);
        b.release(x);
        b.release(skip);
        return 0;
    }

    // ResnetBlock2D / sgm ResnetBlock (model.py:342-362) in two launches: conv1 = GN1+SiLU+conv+temb, conv2 =
    // GN2+SiLU+conv with the shortcut (1x1 conv or identity) as the residual K-phase.  Releases one reference of x and skip.
    int resnet(Builder& b, const std::string& p, Tensor x, Tensor skip, Tensor* out) {
        if (wide_concat(b, x, skip)) return resnet_wide(b, p, x, skip, out);
        ConvArgs c1;
        c1.layer = layers.get_conv(p + ".conv1");
        c1.x0 = x; c1.x1 = skip;
        c1.gn = layers.get_norm(p + ".norm1");
        c1.eps = eps; c1.groups = groups; c1.silu = 1;
        auto it = temb_off.find(p);
        c1.temb_off = it == temb_off.end() ? -1 : it->second;
        c1.want_stats = true;
        Tensor h1;
        if (b.conv(c1, &h1)) return 1;
        ConvArgs c2;
        c2.layer = layers.get_conv(p + ".conv2");
        c2.x0 = h1;
        c2.gn = layers.get_norm(p + ".norm2");
        c2.eps = eps; c2.groups = groups; c2.silu = 1;
        c2.r0 = x; c2.r1 = skip;
        c2.want_stats = true;
        if (b.conv(c2, out)) return 1;
        b.release(h1);
        b.release(x);
        b.release(skip);
        return 0;
    }

    // diffusers Attention (+x residual): qkv = GN + Linear(C, 3C); softmax(q k^T / sqrt(8)) v per head; to_out + x.
    // Releases one reference of x.
    // per-head q/k/v fragments for attention_qkv_d8_kernel, built once per layer from the merged qkv Linear
    struct AttnFused {
        DevBuf w, bias;
    };
    std::map<std::string, std::unique_ptr<AttnFused>> attn_fused;
    int get_attn_fused(const std::string& p, int C, AttnFused** out) {
        auto it = attn_fused.find(p);
        if (it != attn_fused.end()) {
            *out = it->second.get();
            return 0;
        }
        ConvLayer* L = layers.get_conv(p + ".qkv");
        RLDM_REQUIRE(L && L->Cin == C && L->Cout == 3 * C, "attention " + p + ": unexpected q/k/v shapes");
        std::vector<bf16_t> img;
        std::vector<float> bias;
        pack_attn_head_frags(L->w.data(), L->b.data(), C, img, bias);
        auto f = std::make_unique<AttnFused>();
        if (upload(f->w, img.data(), img.size() * sizeof(bf16_t))) return 1;
        if (upload(f->bias, bias.data(), bias.size() * sizeof(float))) return 1;
        *out = f.get();
        attn_fused[p] = std::move(f);
        return 0;
    }

    int attention(Builder& b, const std::string& p, Tensor x, Tensor* out) {
        const int Lt = x.W * x.H;
        if (x.C % 16 == 0 && x.C <= 512 && Lt <= 1024 && x.P > 0 && x.C % groups == 0) {
            // GroupNorm + q/k/v projection inside the attention launch: no [B][L][3C] tensor, one launch less
            NormParams* gnp = layers.get_norm(p + ".group_norm");
            b.record_consumer(gnp, x, Tensor(), 0, true, groups, eps);
            Tensor xn;                                  // x already normalised by its producer (producer-side GroupNorm)
            const bool pre = b.take_view(gnp, &xn);
            Tensor o = b.make(x.B, x.W, x.H, x.C);
            const double fl = 4.0 * (double)x.B * (x.C / 8) * (double)Lt * Lt * 8 + 2.0 * (double)x.B * Lt * 3.0 * x.C * x.C;
            b.plan->flops += fl;
            bool in_trunk = b.trunk_attention_ok(x, pre);           // a phase of the persistent trunk launch (trunk.hip)
            const int cl_ranks = in_trunk ? 0 : b.cluster_attention_ranks(x, pre);
            if (in_trunk) b.trunk_begin(x.B, x.C / b.own_tile_channels(x.B, Lt, x.C));
            else if (cl_ranks) b.trunk_begin(x.B, cl_ranks, x.C / 64, 2);
            else b.note_launch();
            in_trunk = in_trunk || cl_ranks != 0;
            // the stand-alone launch also carries the block's output projection (+ x, + statistics) when an image's workgroups are
            // 64-pixel blocks of it on one XCD, all resident: the 128x8 level at batch 8 / 16 (attention_body.h, attention_proj_tail);
            // RLDM_FLAG_ATTN_PROJ_LAUNCH keeps the projection a launch of its own
            // (without clusters -- a sampler's per-layer fall-back, several chains, the routing switches -- the SAME tail runs as a launch of
            //  its own behind the attention launch: identical results)
            const bool proj_tail = !in_trunk && !(dbg() & RLDM_FLAG_ATTN_PROJ_LAUNCH) && attention_proj_fusable(x.B, Lt, x.C, -1);
            const bool proj_seam = proj_tail && b.cluster_enabled() &&
                                   attention_proj_fusable(x.B, Lt, x.C, Builder::device_cus() / std::max(1, b.concurrent_plans));
            const bool fuse_proj = proj_tail;
            Tensor yfused;
            if (fuse_proj) {
                yfused = b.make(x.B, x.W, x.H, x.C);
                b.add_stats(yfused, Lt / 64);
            }
            if (!b.dry) {
                AttnFused* f = nullptr;
                if (get_attn_fused(p, x.C, &f)) return 1;
                AttnQkvParams ap;
                memset(&ap, 0, sizeof(ap));
                ap.x = pre ? b.tptr(xn) : b.tptr(x);
                ap.st = pre ? nullptr : b.sptr(x);
                ap.P = x.P;
                ap.gamma = gnp->gamma.as<float>();
                ap.beta = gnp->beta.as<float>();
                ap.eps = eps;
                ap.groups = groups;
                const int cpg = x.C / groups;
                ap.inv_n = (float)(1.0 / ((double)Lt * cpg));
                ap.magic_cpg = ((1 << 20) + cpg - 1) / cpg;
                ap.wfrag = f->w.as<bf16_t>();
                ap.bias = f->bias.as<float>();
                ap.out = b.tptr(o);
                ap.B = x.B; ap.L = Lt; ap.C = x.C;
                ap.ts = stamp_buf(StampSite::Attn);
                ap.ts_L = stamp_env().attn_l ? atoi(stamp_env().attn_l) : 0;
                double by = (double)x.B * Lt * x.C * 2.0 * 2.0 + 3.0 * x.C * x.C * 2.0;
                double flp = fl;
                if (fuse_proj) {
                    ConvLayer* Lo = layers.get_conv(p + ".to_out.0");
                    ConvLayer::Packed* pk = nullptr;
                    RLDM_REQUIRE(Lo && Lo->Cin == x.C && Lo->Cout == x.C && Lo->sc_identity, "attention " + p + ": unexpected to_out");
                    if (Lo->get_fragpacked(x.C, 32, 1, true, &pk)) return 1;
                    ap.proj_w = pk->w.as<bf16_t>();
                    ap.proj_bias = pk->bias.as<float>();
                    ap.proj_res = b.tptr(x);
                    ap.proj_y = b.tptr(yfused);
                    ap.proj_stats = b.ptr<float2>(yfused.st_off);
                    if (proj_seam) {
                        auto ctrs = std::make_unique<DevBuf>();
                        if (ctrs->alloc((size_t)x.B * 32 * 4)) return 1;
                        RLDM_HIP_CHECK(hipMemset(ctrs->p, 0, ctrs->bytes));
                        if (!b.plan->trunk_error.p) {
                            if (b.plan->trunk_error.alloc(64)) return 1;
                            RLDM_HIP_CHECK(hipMemset(b.plan->trunk_error.p, 0, 64));
                        }
                        ap.proj_counter = ctrs->as<unsigned>();
                        ap.proj_error = b.plan->trunk_error.as<int>();
                        b.plan->trunk_bufs.push_back(std::move(ctrs));
                        flp += 2.0 * (double)x.B * Lt * x.C * x.C;
                        by += (double)x.B * Lt * x.C * 2.0 * 3.0 + (double)x.C * x.C * 2.0;
                    }
                }
                Op standalone{[ap](hipStream_t s) { return launch_attention_qkv(ap, s); },
                              proj_seam ? "attention_qkv_d8_kernel + to_out" : "attention_qkv_d8_kernel", flp, by};
                standalone.tag = p;
                if (in_trunk) {
                    b.trunk_push_attention(ap, fl, by);
                    b.pend.standalone.push_back(standalone);
                } else {
                    b.plan->ops.push_back(standalone);
                }
                if (fuse_proj && !proj_seam) {          // the tail as its own launch (no seam: the kernel boundary orders it)
                    Op tail{[ap](hipStream_t s) { return launch_attention_proj(ap, s); }, "attention_proj_kernel",
                            2.0 * (double)x.B * Lt * x.C * x.C, (double)x.B * Lt * x.C * 2.0 * 3.0 + (double)x.C * x.C * 2.0};
                    tail.tag = p + ".to_out.0";
                    b.plan->ops.push_back(tail);
                }
            }
            if (fuse_proj && !proj_seam) b.note_launch();
            if (pre) b.release(xn);
            if (fuse_proj) {
                b.plan->flops += 2.0 * (double)x.B * Lt * x.C * x.C;
                b.release(o);
                b.release(x);
                *out = yfused;
                return 0;
            }
            ConvArgs co;
            co.layer = layers.get_conv(p + ".to_out.0");
            co.x0 = o;
            co.r0 = x;
            co.want_stats = true;
            if (b.conv(co, out)) return 1;
            b.release(o);
            b.release(x);
            return 0;
        }
        ConvArgs cq;
        cq.layer = layers.get_conv(p + ".qkv");
        cq.x0 = x;
        cq.gn = layers.get_norm(p + ".group_norm");
        cq.eps = eps; cq.groups = groups; cq.silu = 0;
        Tensor qkv;
        if (b.conv(cq, &qkv)) return 1;
        Tensor o = b.make(x.B, x.W, x.H, x.C);
        const int L = x.W * x.H;
        b.plan->flops += 4.0 * (double)x.B * (x.C / 8) * (double)L * L * 8;
        b.note_launch();
        if (!b.dry) {
            AttnParams ap;
            ap.qkv = b.tptr(qkv); ap.out = b.tptr(o);
            ap.B = x.B; ap.L = L; ap.C = x.C;
            b.plan->ops.push_back({[ap](hipStream_t s) { return launch_attention(ap, s); }, "attention_d8_kernel",
                                   4.0 * (double)x.B * (x.C / 8) * (double)L * L * 8, (double)x.B * L * x.C * 2.0 * 4.0});
        }
        b.release(qkv);
        ConvArgs co;
        co.layer = layers.get_conv(p + ".to_out.0");
        co.x0 = o;
        co.r0 = x;
        co.want_stats = true;
        if (b.conv(co, out)) return 1;
        b.release(o);
        b.release(x);
        return 0;
    }

    int add_resnet(ParamStore& ps, const std::string& p, int ci, int co, bool temb) {
        if (layers.add_norm(ps, p + ".norm1", ci)) return 1;
        if (layers.add_conv(ps, p + ".conv1", co, ci, 3)) return 1;
        if (layers.add_norm(ps, p + ".norm2", co)) return 1;
        if (layers.add_conv(ps, p + ".conv2", co, co, 3)) return 1;
        ConvLayer* c2 = layers.get_conv(p + ".conv2");
        if (ci != co) {                              // conv_shortcut(x) folded into conv2: weights appended, biases summed
            c2->R = ci;
            c2->sc_w = ps.host.at(p + ".conv_shortcut.weight");
            const auto& sb = ps.host.at(p + ".conv_shortcut.bias");
            for (int i = 0; i < co; ++i) c2->b[i] += sb[i];
        } else {
            c2->R = co;
            c2->sc_identity = true;
        }
        if (temb) {
            temb_off[p] = temb_ld;
            temb_ld += co;
        }
        return 0;
    }
    int add_attn(ParamStore& ps, const std::string& p, int c, int head_dim) {
        if (layers.add_norm(ps, p + ".group_norm", c)) return 1;
        if (layers.add_qkv(ps, p, c, head_dim)) return 1;
        if (layers.add_conv(ps, p + ".to_out.0", c, c, 1)) return 1;
        ConvLayer* o = layers.get_conv(p + ".to_out.0");
        o->R = c;
        o->sc_identity = true;
        return 0;
    }
};

}  // namespace rldm

using namespace rldm;

// =================================================================================================================
// UNet2DModel
// =================================================================================================================
// (runtime.h declares the objects; NetCommon is complete only here, so they are made and destroyed here)
rldm_unet::rldm_unet() : net(std::make_unique<NetCommon>()) {}
rldm_unet::~rldm_unet() = default;
rldm_vae::rldm_vae() : net(std::make_unique<NetCommon>()) {}
rldm_vae::~rldm_vae() = default;
int rldm::unet_temb_ld(const rldm_unet* m) { return m->net->temb_ld; }
int rldm::unet_temb_off(const rldm_unet* m, const std::string& resnet_prefix) {
    auto it = m->net->temb_off.find(resnet_prefix);
    return it == m->net->temb_off.end() ? -1 : it->second;
}

static void unet_expect(rldm_unet* m) {
    const auto& c = m->cfg;
    ParamStore& ps = m->params;
    const int* boc = c.block_out_channels;
    const int L = c.num_levels;
    const int temb = boc[0] * 4;
    ps.expect_conv("conv_in", boc[0], c.in_channels, 3);
    ps.expect_lin("time_embedding.linear_1", temb, boc[0]);
    ps.expect_lin("time_embedding.linear_2", temb, temb);
    int out = boc[0];
    for (int i = 0; i < L; ++i) {
        int cin = out;
        out = boc[i];
        for (int j = 0; j < c.layers_per_block; ++j) {
            ps.expect_resnet("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? cin : out, out, temb);
            if (c.down_attn[i]) ps.expect_attn("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), out);
        }
        if (i != L - 1) ps.expect_conv("down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out, out, 3);
    }
    const int cm = boc[L - 1];
    ps.expect_resnet("mid_block.resnets.0", cm, cm, temb);
    if (c.mid_attention) ps.expect_attn("mid_block.attentions.0", cm);
    ps.expect_resnet("mid_block.resnets.1", cm, cm, temb);
    out = boc[L - 1];
    for (int i = 0; i < L; ++i) {
        const int prev = out;
        out = boc[L - 1 - i];
        const int inp = boc[L - 1 - std::min(i + 1, L - 1)];
        const int n = c.layers_per_block + 1;
        for (int j = 0; j < n; ++j) {
            const int skip = (j == n - 1) ? inp : out;
            const int rin = (j == 0) ? prev : out;
            ps.expect_resnet("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), rin + skip, out, temb);
            if (c.up_attn[i]) ps.expect_attn("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), out);
        }
        if (i != L - 1) ps.expect_conv("up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out, out, 3);
    }
    ps.expect_norm("conv_norm_out", boc[0]);
    ps.expect_conv("conv_out", c.out_channels, boc[0], 3);
}

static int unet_build_layers(rldm_unet* m) {
    const auto& c = m->cfg;
    ParamStore& ps = m->params;
    NetCommon& net = *m->net;
    net = NetCommon();
    net.groups = c.norm_num_groups;
    net.eps = c.norm_eps;
    const int* boc = c.block_out_channels;
    const int L = c.num_levels;
    const int hd = c.attention_head_dim;
    m->temb_dim = boc[0] * 4;
    if (net.layers.add_conv(ps, "conv_in", boc[0], c.in_channels, 3)) return 1;
    int out = boc[0];
    for (int i = 0; i < L; ++i) {
        int cin = out;
        out = boc[i];
        for (int j = 0; j < c.layers_per_block; ++j) {
            const std::string r = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            if (net.add_resnet(ps, r, j == 0 ? cin : out, out, true)) return 1;
            m->resnet_order.push_back(r);
            if (c.down_attn[i] && net.add_attn(ps, "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), out, hd)) return 1;
        }
        if (i != L - 1 && net.layers.add_conv(ps, "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out, out, 3)) return 1;
    }
    const int cm = boc[L - 1];
    if (net.add_resnet(ps, "mid_block.resnets.0", cm, cm, true)) return 1;
    m->resnet_order.push_back("mid_block.resnets.0");
    if (c.mid_attention && net.add_attn(ps, "mid_block.attentions.0", cm, hd)) return 1;
    if (net.add_resnet(ps, "mid_block.resnets.1", cm, cm, true)) return 1;
    m->resnet_order.push_back("mid_block.resnets.1");
    out = boc[L - 1];
    for (int i = 0; i < L; ++i) {
        const int prev = out;
        out = boc[L - 1 - i];
        const int inp = boc[L - 1 - std::min(i + 1, L - 1)];
        const int n = c.layers_per_block + 1;
        for (int j = 0; j < n; ++j) {
            const int skip = (j == n - 1) ? inp : out;
            const int rin = (j == 0) ? prev : out;
            const std::string r = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            if (net.add_resnet(ps, r, rin + skip, out, true)) return 1;
            m->resnet_order.push_back(r);
            if (c.up_attn[i] && net.add_attn(ps, "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), out, hd)) return 1;
        }
        if (i != L - 1 && net.layers.add_conv(ps, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out, out, 3)) return 1;
    }
    if (net.layers.add_norm(ps, "conv_norm_out", boc[0])) return 1;
    if (net.layers.add_conv(ps, "conv_out", c.out_channels, boc[0], 3)) return 1;

    // time-embedding weights (fp32): linear_1, linear_2, all time_emb_proj concatenated in resnet order
    const int D = m->temb_dim;
    if (upload(m->w1, ps.host.at("time_embedding.linear_1.weight").data(), (size_t)D * boc[0] * 4)) return 1;
    if (upload(m->b1, ps.host.at("time_embedding.linear_1.bias").data(), (size_t)D * 4)) return 1;
    if (upload(m->w2, ps.host.at("time_embedding.linear_2.weight").data(), (size_t)D * D * 4)) return 1;
    if (upload(m->b2, ps.host.at("time_embedding.linear_2.bias").data(), (size_t)D * 4)) return 1;
    std::vector<float> wp((size_t)net.temb_ld * D), bp(net.temb_ld);
    for (auto& r : m->resnet_order) {
        const int off = net.temb_off.at(r);
        const auto& w = ps.host.at(r + ".time_emb_proj.weight");
        const auto& b = ps.host.at(r + ".time_emb_proj.bias");
        std::copy(w.begin(), w.end(), wp.begin() + (size_t)off * D);
        std::copy(b.begin(), b.end(), bp.begin() + off);
    }
    if (upload(m->wp, wp.data(), wp.size() * 4)) return 1;
    if (upload(m->bp, bp.data(), bp.size() * 4)) return 1;
    return 0;
}

// one pass of the UNet walk (dry: sizes only)
static int unet_walk(rldm_unet* m, Builder& b, int B) {
    const auto& c = m->cfg;
    NetCommon& net = *m->net;
    const int L = c.num_levels;
    const int W = c.sample_w, H = c.sample_h;
    const int Cpad = pad16(c.in_channels);
    Plan* plan = b.plan;

    Tensor xin = b.make(B, W, H, Cpad);
    b.note_launch();
    if (!b.dry) {
        bf16_t* dst = b.tptr(xin);
        plan->io.xin = dst;
        plan->io.xin_ld = Cpad;
        plan->ops.push_back({[plan, dst, B, W, H, Cpad](hipStream_t s) {
            if (plan->io.pack_fused) return 0;          // (the sampler packed x_T; afterwards conv_out's epilogue writes this tensor)
            PackInputParams p{};
            p.x = plan->io.sample; p.cx = plan->io.sample_channels; p.scale = plan->io.sample_scale;
            p.pos_encoding = plan->io.pos_encoding;
            p.cond = plan->io.cond; p.cc = plan->io.cond_channels;
            p.B = B; p.W = W; p.H = H; p.Cpad = Cpad;
            p.out = dst;
            p.step_inc = plan->io.step_inc;
            return launch_pack_input(p, s);
        }, "pack_input_kernel", 0.0, (double)B * W * H * (Cpad * 2.0 + 4.0 * 5), [plan]() { return !plan->io.pack_fused; }});
    }
    Tensor h;
    {
        ConvArgs a;
        a.layer = net.layers.get_conv("conv_in");
        a.x0 = xin;
        a.want_stats = true;
        a.first_of_step = true;
        if (b.conv(a, &h)) return 1;
        // (xin is never released: with the pack launch fused away it must survive from conv_out's epilogue to the next step's conv_in)
    }
    std::vector<Tensor> skips;
    b.retain(h);
    skips.push_back(h);
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j) {
            Tensor o;
            if (net.resnet(b, "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), h, Tensor(), &o)) return 1;
            h = o;
            if (c.down_attn[i]) {
                if (net.attention(b, "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), h, &o)) return 1;
                h = o;
            }
            b.retain(h);
            skips.push_back(h);
        }
        if (i != L - 1) {
            ConvArgs a;
            a.layer = net.layers.get_conv("down_blocks." + std::to_string(i) + ".downsamplers.0.conv");
            a.x0 = h;
            a.stride = 2;
            a.want_stats = true;
            Tensor o;
            if (b.conv(a, &o)) return 1;
            b.release(h);
            h = o;
            b.retain(h);
            skips.push_back(h);
        }
    }
    {
        Tensor o;
        if (net.resnet(b, "mid_block.resnets.0", h, Tensor(), &o)) return 1;
        h = o;
        if (c.mid_attention) {
            if (net.attention(b, "mid_block.attentions.0", h, &o)) return 1;
            h = o;
        }
        if (net.resnet(b, "mid_block.resnets.1", h, Tensor(), &o)) return 1;
        h = o;
    }
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            RLDM_REQUIRE(!skips.empty(), "internal: skip stack underflow");
            Tensor sk = skips.back();
            skips.pop_back();
            Tensor o;
            if (net.resnet(b, "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), h, sk, &o)) return 1;
            h = o;
            if (c.up_attn[i]) {
                if (net.attention(b, "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), h, &o)) return 1;
                h = o;
            }
        }
        if (i != L - 1) {
            ConvArgs a;
            a.layer = net.layers.get_conv("up_blocks." + std::to_string(i) + ".upsamplers.0.conv");
            a.x0 = h;
            a.up = 2;
            a.want_stats = true;
            Tensor o;
            if (b.conv(a, &o)) return 1;
            b.release(h);
            h = o;
        }
    }
    RLDM_REQUIRE(skips.empty(), "internal: skip stack not drained");
    {
        ConvArgs a;
        a.layer = net.layers.get_conv("conv_out");
        a.x0 = h;
        a.gn = net.layers.get_norm("conv_norm_out");
        a.eps = net.eps; a.groups = net.groups; a.silu = 1;
        a.out_f32_nchw = true;
        Tensor none;
        if (b.conv(a, &none)) return 1;
        b.release(h);
    }
    return 0;
}

int rldm::unet_make_plan(rldm_unet* m, int B, std::unique_ptr<Plan>* out, int* launches, int flags, int concurrent_plans) {
    auto plan = std::make_unique<Plan>();
    plan->B = B; plan->W = m->cfg.sample_w; plan->H = m->cfg.sample_h;
    plan->flags = flags;
    if (build_plan(plan.get(), m->net->temb_ld, [&](Builder& b) { return unet_walk(m, b, B); }, launches, concurrent_plans)) return 1;
    *out = std::move(plan);
    return 0;
}

// time-embedding table for `rows` timesteps (host floats) into `tab`
int rldm::unet_temb(rldm_unet* m, const float* t_dev, int rows, float* tab, hipStream_t s) {
    TembParams p;
    p.t = t_dev; p.rows = rows;
    p.dim0 = m->cfg.block_out_channels[0]; p.D = m->temb_dim; p.total = m->net->temb_ld;
    p.w1 = m->w1.as<float>(); p.b1 = m->b1.as<float>();
    p.w2 = m->w2.as<float>(); p.b2 = m->b2.as<float>();
    p.wp = m->wp.as<float>(); p.bp = m->bp.as<float>();
    p.out = tab;
    const size_t need = (size_t)2 * rows * m->temb_dim * sizeof(float);
    if (m->temb_scratch.bytes < need && m->temb_scratch.alloc(need)) return 1;
    p.scratch = m->temb_scratch.as<float>();
    p.flip_sin_to_cos = m->cfg.flip_sin_to_cos; p.freq_shift = m->cfg.freq_shift;
    return launch_temb(p, s);
}

// =================================================================================================================
// VAE
// =================================================================================================================
static void vae_expect(rldm_vae* m) {
    const auto& c = m->cfg;
    ParamStore& ps = m->params;
    const int L = c.num_levels;
    std::vector<int> chs(L);
    for (int i = 0; i < L; ++i) chs[i] = c.ch * c.ch_mult[i];
    ps.expect_conv("encoder.conv_in", c.ch, c.in_channels, 3);
    int cin = c.ch;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.num_res_blocks; ++j) {
            ps.expect_resnet("encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cin, chs[i], 0);
            cin = chs[i];
        }
        if (i != L - 1) ps.expect_conv("encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", cin, cin, 3);
    }
    ps.expect_resnet("encoder.mid_block.resnets.0", cin, cin, 0);
    ps.expect_resnet("encoder.mid_block.resnets.1", cin, cin, 0);
    ps.expect_norm("encoder.conv_norm_out", cin);
    ps.expect_conv("encoder.conv_out", c.double_z ? 2 * c.z_channels : c.z_channels, cin, 3);
    cin = chs[L - 1];
    ps.expect_conv("decoder.conv_in", cin, c.z_channels, 3);
    ps.expect_resnet("decoder.mid_block.resnets.0", cin, cin, 0);
    ps.expect_resnet("decoder.mid_block.resnets.1", cin, cin, 0);
    for (int i = 0; i < L; ++i) {
        const int cout = chs[L - 1 - i];
        for (int j = 0; j < c.num_res_blocks + 1; ++j) {
            ps.expect_resnet("decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cin, cout, 0);
            cin = cout;
        }
        if (i != L - 1) ps.expect_conv("decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", cin, cin, 3);
    }
    ps.expect_norm("decoder.conv_norm_out", cin);
    ps.expect_conv("decoder.conv_out", c.out_channels, cin, 3);
}

static int vae_build_layers(rldm_vae* m) {
    const auto& c = m->cfg;
    ParamStore& ps = m->params;
    NetCommon& net = *m->net;
    net = NetCommon();
    net.groups = c.norm_num_groups;
    net.eps = c.norm_eps;
    const int L = c.num_levels;
    std::vector<int> chs(L);
    for (int i = 0; i < L; ++i) chs[i] = c.ch * c.ch_mult[i];
    if (net.layers.add_conv(ps, "encoder.conv_in", c.ch, c.in_channels, 3)) return 1;
    int cin = c.ch;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.num_res_blocks; ++j) {
            if (net.add_resnet(ps, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cin, chs[i], false)) return 1;
            cin = chs[i];
        }
        if (i != L - 1 && net.layers.add_conv(ps, "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", cin, cin, 3)) return 1;
    }
    if (net.add_resnet(ps, "encoder.mid_block.resnets.0", cin, cin, false)) return 1;
    if (net.add_resnet(ps, "encoder.mid_block.resnets.1", cin, cin, false)) return 1;
    if (net.layers.add_norm(ps, "encoder.conv_norm_out", cin)) return 1;
    if (net.layers.add_conv(ps, "encoder.conv_out", c.double_z ? 2 * c.z_channels : c.z_channels, cin, 3)) return 1;
    cin = chs[L - 1];
    if (net.layers.add_conv(ps, "decoder.conv_in", cin, c.z_channels, 3)) return 1;
    if (net.add_resnet(ps, "decoder.mid_block.resnets.0", cin, cin, false)) return 1;
    if (net.add_resnet(ps, "decoder.mid_block.resnets.1", cin, cin, false)) return 1;
    for (int i = 0; i < L; ++i) {
        const int cout = chs[L - 1 - i];
        for (int j = 0; j < c.num_res_blocks + 1; ++j) {
            if (net.add_resnet(ps, "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cin, cout, false)) return 1;
            cin = cout;
        }
        if (i != L - 1 && net.layers.add_conv(ps, "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", cin, cin, 3)) return 1;
    }
    if (net.layers.add_norm(ps, "decoder.conv_norm_out", cin)) return 1;
    if (net.layers.add_conv(ps, "decoder.conv_out", c.out_channels, cin, 3)) return 1;
    return 0;
}

static void push_pack_input(Builder& b, Tensor xin) {
    b.note_launch();
    if (b.dry) return;
    Plan* plan = b.plan;
    bf16_t* dst = b.tptr(xin);
    const int B = xin.B, W = xin.W, H = xin.H, Cpad = xin.C;
    plan->ops.push_back({[plan, dst, B, W, H, Cpad](hipStream_t s) {
        PackInputParams p{};
        p.x = plan->io.sample; p.cx = plan->io.sample_channels; p.scale = plan->io.sample_scale;
        p.pos_encoding = 0; p.cond = nullptr; p.cc = 0;
        p.B = B; p.W = W; p.H = H; p.Cpad = Cpad;
        p.out = dst;
        return launch_pack_input(p, s);
    }, "pack_input_kernel", 0.0, (double)B * W * H * (Cpad * 2.0 + 4.0 * 4)});
}

static int vae_walk_decode(rldm_vae* m, Builder& b, int B, int w, int h) {
    const auto& c = m->cfg;
    NetCommon& net = *m->net;
    const int L = c.num_levels;
    Tensor xin = b.make(B, w, h, pad16(c.z_channels));
    push_pack_input(b, xin);
    Tensor t;
    ConvArgs a;
    a.layer = net.layers.get_conv("decoder.conv_in");
    a.x0 = xin;
    a.want_stats = true;
    if (b.conv(a, &t)) return 1;
    b.release(xin);
    Tensor o;
    if (net.resnet(b, "decoder.mid_block.resnets.0", t, Tensor(), &o)) return 1;
    t = o;
    if (net.resnet(b, "decoder.mid_block.resnets.1", t, Tensor(), &o)) return 1;
    t = o;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.num_res_blocks + 1; ++j) {
            if (net.resnet(b, "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), t, Tensor(), &o)) return 1;
            t = o;
        }
        if (i != L - 1) {
            ConvArgs u;
            u.layer = net.layers.get_conv("decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv");
            u.x0 = t;
            u.up = 2;
            u.want_stats = true;
            if (b.conv(u, &o)) return 1;
            b.release(t);
            t = o;
        }
    }
    ConvArgs co;
    co.layer = net.layers.get_conv("decoder.conv_out");
    co.x0 = t;
    co.gn = net.layers.get_norm("decoder.conv_norm_out");
    co.eps = net.eps; co.groups = net.groups; co.silu = 1;
    co.out_f32_nchw = true;
    Tensor none;
    if (b.conv(co, &none)) return 1;
    b.release(t);
    return 0;
}

static int vae_walk_encode(rldm_vae* m, Builder& b, int B, int w, int h) {
    const auto& c = m->cfg;
    NetCommon& net = *m->net;
    const int L = c.num_levels;
    Tensor xin = b.make(B, w, h, pad16(c.in_channels));
    push_pack_input(b, xin);
    Tensor t;
    ConvArgs a;
    a.layer = net.layers.get_conv("encoder.conv_in");
    a.x0 = xin;
    a.want_stats = true;
    if (b.conv(a, &t)) return 1;
    b.release(xin);
    Tensor o;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < c.num_res_blocks; ++j) {
            if (net.resnet(b, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), t, Tensor(), &o)) return 1;
            t = o;
        }
        if (i != L - 1) {
            ConvArgs d;
            d.layer = net.layers.get_conv("encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv");
            d.x0 = t;
            d.stride = 2;
            d.want_stats = true;
            d.pad_mode = 1;                          // end-only pad: ldm/utils.py:109-111, model.py:164-172
            if (b.conv(d, &o)) return 1;
            b.release(t);
            t = o;
        }
    }
    if (net.resnet(b, "encoder.mid_block.resnets.0", t, Tensor(), &o)) return 1;
    t = o;
    if (net.resnet(b, "encoder.mid_block.resnets.1", t, Tensor(), &o)) return 1;
    t = o;
    ConvArgs co;
    co.layer = net.layers.get_conv("encoder.conv_out");
    co.x0 = t;
    co.gn = net.layers.get_norm("encoder.conv_norm_out");
    co.eps = net.eps; co.groups = net.groups; co.silu = 1;
    co.out_f32_nchw = true;
    Tensor none;
    if (b.conv(co, &none)) return 1;
    b.release(t);
    return 0;
}

int rldm::vae_make_plan(rldm_vae* m, int B, int w, int h, bool enc, std::unique_ptr<Plan>* out, int flags) {
    auto plan = std::make_unique<Plan>();
    plan->B = B; plan->W = w; plan->H = h;
    plan->flags = flags;
    if (build_plan(plan.get(), 0, [&](Builder& b) { return enc ? vae_walk_encode(m, b, B, w, h) : vae_walk_decode(m, b, B, w, h); }))
        return 1;
    *out = std::move(plan);
    return 0;
}

static int vae_get_plan(rldm_vae* m, int B, int w, int h, bool enc, Plan** out) {
    rldm_vae::Key k{B, w, h, enc ? 1 : 0};
    auto it = m->plans.find(k);
    if (it == m->plans.end()) {
        std::unique_ptr<Plan> p;
        if (vae_make_plan(m, B, w, h, enc, &p)) return 1;
        it = m->plans.emplace(k, std::move(p)).first;
    }
    *out = it->second.get();
    return 0;
}

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

const char* rldm_last_error(void) { return g_error.c_str(); }

int rldm_device_info(char* name, size_t name_len, int* compute_units) {
    int n = 0;
    RLDM_HIP_CHECK(hipGetDeviceCount(&n));
    RLDM_REQUIRE(n > 0, "no HIP device visible");
    int dev = 0;
    RLDM_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    RLDM_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (name && name_len) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    RLDM_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
                 std::string("librangeldm_hip is built for gfx950 only; device is ") + prop.gcnArchName);
    return 0;
}

// ---- UNet -------------------------------------------------------------------------------------------------------
int rldm_unet_create(const rldm_unet_config* cfg, rldm_unet** out) {
    RLDM_REQUIRE(cfg && out, "null argument");
    RLDM_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= RLDM_MAX_LEVELS, "num_levels out of range");
    RLDM_REQUIRE(cfg->attention_head_dim == 8, "only attention_head_dim == 8 (the UNet2DModel default the reference uses) is supported");
    RLDM_REQUIRE(cfg->in_channels <= 16, "in_channels > 16 not supported");
    for (int i = 0; i < cfg->num_levels; ++i)
        RLDM_REQUIRE(cfg->block_out_channels[i] % 32 == 0 && cfg->block_out_channels[i] <= 512,
                     "block_out_channels must be multiples of 32, <= 512");
    RLDM_REQUIRE((cfg->sample_w >> (cfg->num_levels - 1)) >= 2 && (cfg->sample_h >> (cfg->num_levels - 1)) >= 1 &&
                     cfg->sample_w % (1 << (cfg->num_levels - 1)) == 0 && cfg->sample_h % (1 << (cfg->num_levels - 1)) == 0,
                 "sample_size not divisible by 2^(levels-1)");
    auto* m = new rldm_unet();
    m->cfg = *cfg;
    unet_expect(m);
    *out = m;
    return 0;
}
void rldm_unet_destroy(rldm_unet* m) { delete m; }

int rldm_unet_set_param(rldm_unet* m, const char* name, const float* data, int64_t numel) {
    RLDM_REQUIRE(m && name && data, "null argument");
    m->plans.clear();
    m->params.finalized = false;                    // a live sampler refuses to run until rldm_unet_finalize rebuilt the weights
    return m->params.set(name, data, numel);
}

int rldm_unet_finalize(rldm_unet* m) {
    RLDM_REQUIRE(m, "null argument");
    if (m->params.check_complete()) return 1;
    m->resnet_order.clear();
    m->plans.clear();
    if (unet_build_layers(m)) return 1;
    m->params.finalized = true;
    ++m->generation;
    return 0;
}

static int unet_get_plan(rldm_unet* m, int B, Plan** out) {
    RLDM_REQUIRE(m->params.finalized, "rldm_unet_finalize has not been called");
    auto it = m->plans.find(B);
    if (it == m->plans.end()) {
        std::unique_ptr<Plan> p;
        if (unet_make_plan(m, B, &p, nullptr, m->plan_flags)) return 1;
        it = m->plans.emplace(B, std::move(p)).first;
        m->trunk_checked.erase(B);
    }
    *out = it->second.get();
    return 0;
}

int rldm_unet_forward(rldm_unet* m, const float* sample, const int64_t* timesteps, int nt, int B, float* out, void* stream) {
    RLDM_REQUIRE(m && sample && timesteps && out, "null argument");
    RLDM_REQUIRE(B >= 1 && (nt == 1 || nt == B), "timesteps must have length 1 or B");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Plan* plan = nullptr;
    if (unet_get_plan(m, B, &plan)) return 1;
    if (m->temb_rows_cap < nt) {
        if (m->t_dev.alloc((size_t)nt * 4)) return 1;
        if (m->temb_tab.alloc((size_t)nt * m->net->temb_ld * 4)) return 1;
        m->temb_rows_cap = nt;
    }
    std::vector<float> tf(nt);
    for (int i = 0; i < nt; ++i) tf[i] = (float)timesteps[i];
    RLDM_HIP_CHECK(hipMemcpyAsync(m->t_dev.p, tf.data(), (size_t)nt * 4, hipMemcpyHostToDevice, st));
    RLDM_HIP_CHECK(hipStreamSynchronize(st));   // tf is a stack-lifetime staging buffer
    if (unet_temb(m, m->t_dev.as<float>(), nt, m->temb_tab.as<float>(), st)) return 1;
    plan->io = PlanIO();
    plan->io.sample = sample;
    plan->io.sample_channels = m->cfg.in_channels;
    plan->io.out = out;
    plan->io.temb = m->temb_tab.as<float>();
    plan->io.step_ptr = nullptr;
    plan->io.temb_rows_per_step = nt;
    plan->io.temb_per_sample = (nt == B && B > 1) ? 1 : 0;
    if (plan->run(st)) return 1;
    if (plan->trunk_error.p && !m->trunk_checked[B]) {
        // first run of a plan with persistent launches: read their self-check word before anybody uses `out` (the sampler does the same
        // at its warm-up step); if it is set, this model's plans are rebuilt as one launch per layer and the forward runs again
        RLDM_HIP_CHECK(hipStreamSynchronize(st));
        int terr = 0;
        RLDM_HIP_CHECK(hipMemcpy(&terr, plan->trunk_error.p, 4, hipMemcpyDeviceToHost));
        if (terr != 0) {
            RLDM_REQUIRE(!((dbg_process() | m->plan_flags) & RLDM_FLAG_NO_PERSISTENT), "internal: self-check word set without persistent launches");
            fprintf(stderr, "librangeldm_hip: persistent launches of rldm_unet_forward failed their self-check (code %d); this model runs "
                            "one launch per layer from here on\n", terr);
            m->plan_flags |= RLDM_FLAG_NO_PERSISTENT;
            m->plans.clear();
            return rldm_unet_forward(m, sample, timesteps, nt, B, out, stream);
        }
        m->trunk_checked[B] = true;
    }
    return 0;
}

double rldm_unet_flops(rldm_unet* m, int B) {
    Plan* plan = nullptr;
    if (!m || unet_get_plan(m, B, &plan)) return -1.0;
    return plan->flops;
}

// self-check word of the persistent trunk launches of the batch-B plan (0 fine / no trunk; 1 a wait gave up; 2 a cluster was spread
// over several XCDs); synchronises the device
int rldm_unet_trunk_status(rldm_unet* m, int B) {
    if (!m) return -1;
    auto it = m->plans.find(B);
    if (it == m->plans.end() || !it->second->trunk_error.p) return 0;
    int terr = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(&terr, it->second->trunk_error.p, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return terr;
}

int rldm_unet_set_plan_flags(rldm_unet* m, int flags) {
    RLDM_REQUIRE(m, "null argument");
    if (flags != m->plan_flags) m->plans.clear();
    m->plan_flags = flags;
    return 0;
}

int rldm_unet_num_launches(rldm_unet* m, int B) {
    if (!m || !m->params.finalized) return -1;
    Plan tmp;                           // build_plan's recording and sizing passes, without the real one
    tmp.flags = m->plan_flags;
    int n = 0;
    if (build_plan(&tmp, m->net->temb_ld, [&](Builder& b) { return unet_walk(m, b, B); }, &n, 1, true)) return -1;
    return n + 1;   // + time-embedding kernel
}

// ---- VAE --------------------------------------------------------------------------------------------------------
int rldm_vae_create(const rldm_vae_config* cfg, rldm_vae** out) {
    RLDM_REQUIRE(cfg && out, "null argument");
    RLDM_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= RLDM_MAX_LEVELS, "num_levels out of range");
    RLDM_REQUIRE(cfg->in_channels <= 16 && cfg->z_channels <= 16, "in/z channels > 16 not supported");
    for (int i = 0; i < cfg->num_levels; ++i)
        RLDM_REQUIRE((cfg->ch * cfg->ch_mult[i]) % 32 == 0 && cfg->ch * cfg->ch_mult[i] <= 512, "ch*mult must be a multiple of 32, <= 512");
    auto* m = new rldm_vae();
    m->cfg = *cfg;
    vae_expect(m);
    *out = m;
    return 0;
}
void rldm_vae_destroy(rldm_vae* m) { delete m; }
int rldm_vae_set_param(rldm_vae* m, const char* name, const float* data, int64_t numel) {
    RLDM_REQUIRE(m && name && data, "null argument");
    m->plans.clear();
    m->params.finalized = false;
    return m->params.set(name, data, numel);
}
int rldm_vae_finalize(rldm_vae* m) {
    RLDM_REQUIRE(m, "null argument");
    if (m->params.check_complete()) return 1;
    m->plans.clear();
    if (vae_build_layers(m)) return 1;
    m->params.finalized = true;
    ++m->generation;
    return 0;
}

int rldm_vae_decode(rldm_vae* m, const float* z, int B, int latent_w, int latent_h, float* image, void* stream) {
    RLDM_REQUIRE(m && z && image, "null argument");
    RLDM_REQUIRE(m->params.finalized, "rldm_vae_finalize has not been called");
    Plan* plan = nullptr;
    if (vae_get_plan(m, B, latent_w, latent_h, false, &plan)) return 1;
    plan->io = PlanIO();
    plan->io.sample = z;
    plan->io.sample_channels = m->cfg.z_channels;
    plan->io.out = image;
    return plan->run(reinterpret_cast<hipStream_t>(stream));
}

int rldm_vae_encode(rldm_vae* m, const float* x, int B, int w, int h, float* moments, void* stream) {
    RLDM_REQUIRE(m && x && moments, "null argument");
    RLDM_REQUIRE(m->params.finalized, "rldm_vae_finalize has not been called");
    Plan* plan = nullptr;
    if (vae_get_plan(m, B, w, h, true, &plan)) return 1;
    plan->io = PlanIO();
    plan->io.sample = x;
    plan->io.sample_channels = m->cfg.in_channels;
    plan->io.out = moments;
    return plan->run(reinterpret_cast<hipStream_t>(stream));
}

double rldm_vae_decode_flops(rldm_vae* m, int B, int latent_w, int latent_h) {
    Plan* plan = nullptr;
    if (!m || !m->params.finalized || vae_get_plan(m, B, latent_w, latent_h, false, &plan)) return -1.0;
    return plan->flops;
}

int rldm_diag_gaussian_sample(const float* moments, const float* noise, float scale, int B, int z, int spatial,
                              float* out, void* stream) {
    RLDM_REQUIRE(moments && noise && out, "null argument");
    return launch_diag_gaussian(moments, noise, scale, B, z, spatial, out, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
