// I2VGen-XL backbone UNet plan (I2VGenXLUNet as the reference extends it with the two ControlNet residual kwargs:
// i2vgen_xl/models/unets/unet_i2vgen_xl.py, constructor :134-322, forward :519-761).  Order of operations:
//   time_proj -> time_embedding, time_proj(fps) -> fps_embedding, summed :576-607 | every ResNet's time projection as ONE small-M linear
//   over the per-clip embedding (broadcast over the clip's frames by the convolutions' rowvec with rows_per_img = F * H * W) |
//   the context matrix [text | image_latents_context_embedding(frame 0) as 64 tokens | context_embedding(image_embeddings) as 4 tokens]
//   :614-635, ONE [Lk][cross] matrix per batch element | the K / V^T projections of it for every cross-attention (project_text_kv) |
//   image_latents -> image_latents_proj_in -> image_latents_temporal_encoder :637-651, written as columns 4..7 of the conv_in operand
//   rows beside the sample :654-655 | conv_in, transformer_in :656-662 | down blocks collecting the skips | mid block | the residuals
//   :681-714 | up blocks | conv_norm_out + SiLU + conv_out, b c f h w in the sample's dtype :750-756.
// Blocks (diffusers unet_3d_blocks.py, v0.27): per layer ResnetBlock2D -> TemporalConvLayer [-> Transformer2DModel (linear
// projections) -> TransformerTemporalModel].  TemporalConvLayer: four times GroupNorm over the clip (b c f h w statistics) + SiLU + a
// (3,1,1) convolution, the identity added by the fourth's epilogue.  TransformerTemporalModel: GroupNorm over the clip, proj_in, one
// BasicTransformerBlock with double_self_attention (both attentions over the F frames of a pixel), GEGLU feed-forward, proj_out + input;
// its tokens (b h w, f, c) are the frame-major rows this library keeps, read through op_temporal_attn: no permutation.
// The spatial cross-attention reads ONE context per batch element: rows are (b, f, p), so it runs as B problems of F * h * w queries
// (run_basic_tb's cross_B); nothing is repeated over the frames.
// Step-invariant cache (ctrl_unet_i2v_set_cond_cache): what depends on encoder_hidden_states, image_latents and image_embeddings only
// -- every cross-attention's K / V^T (and with them the context matrix, their only reader) and the four encoded latent channels --
// is kept by a KEEP forward in plan-owned buffers and read by REUSE forwards, which skip the stems.
// Activations are frame-major channels-last [(b f) h w][C]; residual streams fp32, fp16 mirrors where a GEMM reads them.  The up path
// never concatenates (as plan_unet_st.cpp).  Main-path operands are split as in plan_unet2d.cpp: the convolutions that carry the WHOLE
// stream rather than a residual branch -- the 1x1 shortcut of every ResNet that changes width, the down- and the up-samplers -- take
// their A operand as [hi | lo] fp16 halves of the fp32 stream, so every fp16 mirror of a stream here is a [hi | lo] row pair, 2 C wide
// (with plain mirrors NARROW measured 1.04e-3 against the 1e-3 bound).  Upsample2D is the implicit GEMM's 9-tap gather (up = 2).
// One stream, no lanes, no grouped launches: capturable as a linear graph.
#include "plan_common.h"
#include <cstdio>

namespace {

constexpr int kPool = 32;                                // image_latents_context_embedding's AdaptiveAvgPool2d((32, 32))
constexpr int kLatTokens = (kPool / 4) * (kPool / 4);    // two stride-2 convolutions behind it: 8 x 8 context tokens
constexpr int kEncWts = 288;                             // op_i2v_latent_encoder's weight block

struct TConvW { Norm n[4]; ConvW c[4]; };                // TemporalConvLayer

struct TTfmW {                   // TransformerTemporalModel, one BasicTransformerBlock with double_self_attention
    Norm norm, ln1, ln2, ln3;
    Lin proj_in, proj_out, ff1, ff2;
    AttnW a1, a2;
    int C = 0, inner = 0;
};

struct STfmW {                   // Transformer2DModel, linear projections, one layer
    Norm norm;
    Lin proj_in, proj_out;
    BasicTBW tb;
    int C = 0;
};

struct IResW { ResnetW r; int toff = 0; };

struct IBlockW {
    std::vector<IResW> res;
    std::vector<TConvW> tconv;
    std::vector<STfmW> attn;     // empty: a block without attention
    std::vector<TTfmW> tattn;
    bool resample = false;
    ConvW conv;                  // downsamplers.0.conv | upsamplers.0.conv
    int Cout = 0;
};

struct UNetI2V : StandalonePlan {
    ctrl_unet_i2v_config cfg{};
    ConvD conv_in, conv_out, pi0, pi1, pi2, ctx0;        // the direct convolutions: stems 4 -> 16 -> 16 -> 4 and 4 -> 32
    ConvW ctx1, ctx2;                                    // 32 -> 64 s2, 64 -> cross s2 (implicit GEMM)
    Lin te1, te2, fe1, fe2, ce1, ce2, temb_cat;
    TTfmW tin;
    std::vector<IBlockW> down, up;
    IBlockW mid;
    Norm norm_out;
    float* enc_part[11] = {};    // the latent encoder's tensors as loaded
    float* enc_w = nullptr;      // ... and as one block (op_i2v_latent_encoder's order)
    int temb_total = 0, n_cross = 0;
    bool split = false;          // CTRL_UNET_SPLIT=1 (plan_unet_st.cpp): split operands for the ResNets' and the temporal convolutions
    KvCache kvc;                 // K / V^T of the context for every cross-attention
    float* lat_keep = nullptr;   // the encoded latent channels [(b f) h w][4] of a KEEP forward
    size_t lat_elems = 0;
    std::vector<void*> lat_retired;
    int key[5] = {0, 0, 0, 0, 0};          // B, F, h, w, text_len the cache was kept for
    std::vector<std::string> temb_names;
    std::vector<int> temb_ns;
    ~UNetI2V() {
        if (lat_keep) (void)hipFree(lat_keep);
        for (void* p : lat_retired) (void)hipFree(p);
    }
};

int validate(const ctrl_unet_i2v_config& c) {
    CTRL_CHECK(c.num_levels >= 1 && c.num_levels <= 4, "unet_i2v: 1 .. 4 levels");
    CTRL_CHECK(c.in_channels == 4, "unet_i2v: in_channels must be 4 (the latent stems and the temporal encoder are built for 4 channels)");
    CTRL_CHECK(c.out_channels >= 1 && c.out_channels <= 4, "unet_i2v: out_channels must be 1 .. 4");
    CTRL_CHECK(c.layers_per_block >= 1 && c.layers_per_block <= 4, "unet_i2v: layers_per_block out of range");
    for (int i = 0; i < c.num_levels; ++i) {
        const int C = c.block_out_channels[i];
        CTRL_CHECK(C >= 64 && C % 64 == 0 && C <= 2048, "unet_i2v: block_out_channels must be multiples of 64 up to 2048 (heads of 64)");
    }
    CTRL_CHECK(c.cross_attention_dim >= 32 && c.cross_attention_dim % 32 == 0, "unet_i2v: cross_attention_dim must be a multiple of 32");
    return 0;
}

int build_res(ParamSink& ps, UNetI2V& t, const std::string& pre, int Cin, int Cout, IResW* w) {
    TRY(build_resnet(ps, pre, Cin, Cout, false, &w->r, t.split, /*shortcut: split, it carries the stream*/ 1));
    w->toff = t.temb_total; t.temb_total += Cout;
    t.temb_names.push_back(pre + ".time_emb_proj"); t.temb_ns.push_back(Cout);
    return 0;
}

int build_tconv(ParamSink& ps, UNetI2V& t, const std::string& pre, int C, TConvW* w) {
    for (int i = 0; i < 4; ++i) {
        const std::string p = pre + ".conv" + std::to_string(i + 1);
        TRY(ps.norm(p + ".0", C, &w->n[i]));
        TRY(ps.conv(p + (i == 0 ? ".2" : ".3"), C, C, 3, /*temporal*/ true, &w->c[i], t.split));     // (conv2..4 hold a Dropout at .2)
    }
    return 0;
}

int build_ttfm(ParamSink& ps, const std::string& pre, int C, int heads, TTfmW* w) {
    const int inner = heads * 64;
    w->C = C; w->inner = inner;
    TRY(ps.norm(pre + ".norm", C, &w->norm));
    TRY(ps.linear(pre + ".proj_in", inner, C, true, false, &w->proj_in));
    const std::string b = pre + ".transformer_blocks.0";
    TRY(ps.norm(b + ".norm1", inner, &w->ln1));
    TRY(build_attn_self(ps, b + ".attn1", inner, heads, 64, &w->a1));
    TRY(ps.norm(b + ".norm2", inner, &w->ln2));
    TRY(build_attn_self(ps, b + ".attn2", inner, heads, 64, &w->a2));       // double_self_attention: to_k / to_v take `inner`
    TRY(ps.norm(b + ".norm3", inner, &w->ln3));
    TRY(ps.linear(b + ".ff.net.0.proj", 8 * inner, inner, true, true, &w->ff1));
    TRY(ps.linear(b + ".ff.net.2", inner, 4 * inner, true, false, &w->ff2));
    TRY(ps.ffn_perm(&w->ff2));
    TRY(ps.linear(pre + ".proj_out", C, inner, true, false, &w->proj_out));
    return 0;
}

int build_stfm(ParamSink& ps, UNetI2V& t, const std::string& pre, int C, STfmW* w) {
    w->C = C;
    TRY(ps.norm(pre + ".norm", C, &w->norm));
    TRY(ps.linear(pre + ".proj_in", C, C, true, false, &w->proj_in));
    TRY(build_basic_tb(ps, pre + ".transformer_blocks.0", C, C / 64, 64, t.cfg.cross_attention_dim, &w->tb));
    TRY(ps.linear(pre + ".proj_out", C, C, true, false, &w->proj_out));
    t.n_cross += 1;
    return 0;
}

// layer j of a block: resnets.j, temp_convs.j [, attentions.j, temp_attentions.j]
int build_layer(ParamSink& ps, UNetI2V& t, IBlockW& b, const std::string& pre, int j, int Cin, bool attn) {
    const std::string js = std::to_string(j);
    TRY(build_res(ps, t, pre + ".resnets." + js, Cin, b.Cout, &b.res[j]));
    TRY(build_tconv(ps, t, pre + ".temp_convs." + js, b.Cout, &b.tconv[j]));
    if (attn) {
        TRY(build_stfm(ps, t, pre + ".attentions." + js, b.Cout, &b.attn[j]));
        TRY(build_ttfm(ps, pre + ".temp_attentions." + js, b.Cout, b.Cout / 64, &b.tattn[j]));
    }
    return 0;
}

int build_unet(ParamSink& ps, UNetI2V& t) {
    const ctrl_unet_i2v_config& c = t.cfg;
    const int nl = c.num_levels, C0 = c.block_out_channels[0], T = 4 * C0, cross = c.cross_attention_dim, ic = c.in_channels;
    t.temb_total = 0; t.n_cross = 0; t.temb_names.clear(); t.temb_ns.clear();
    t.split = policy_is1(P_UNET_SPLIT);
    TRY(ps.conv_direct("conv_in", C0, 2 * ic, &t.conv_in));
    TRY(build_ttfm(ps, "transformer_in", C0, 8, &t.tin));                  // always 8 heads of 64
    TRY(ps.conv_direct("image_latents_proj_in.0", 4 * ic, 4, &t.pi0));
    TRY(ps.conv_direct("image_latents_proj_in.2", 4 * ic, 4 * ic, &t.pi1));
    TRY(ps.conv_direct("image_latents_proj_in.4", ic, 4 * ic, &t.pi2));
    {
        const std::string e = "image_latents_temporal_encoder.";
        const char* names[11] = {"norm1.weight", "norm1.bias", "attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight",
                                 "attn1.to_out.0.weight", "attn1.to_out.0.bias", "ff.net.0.proj.weight", "ff.net.0.proj.bias",
                                 "ff.net.2.weight", "ff.net.2.bias"};
        const std::vector<int64_t> shapes[11] = {{ic}, {ic}, {2 * ic, ic}, {2 * ic, ic}, {2 * ic, ic}, {ic, 2 * ic}, {ic}, {4 * ic, ic}, {4 * ic},
                                                 {ic, 4 * ic}, {ic}};
        for (int i = 0; i < 11; ++i) TRY(ps.raw_f32(e + names[i], shapes[i], &t.enc_part[i]));
    }
    TRY(ps.conv_direct("image_latents_context_embedding.0", 8 * ic, 4, &t.ctx0));
    TRY(ps.conv("image_latents_context_embedding.3", 16 * ic, 8 * ic, 3, false, &t.ctx1));
    TRY(ps.conv("image_latents_context_embedding.5", cross, 16 * ic, 3, false, &t.ctx2));
    TRY(ps.linear("time_embedding.linear_1", T, C0, true, false, &t.te1));
    TRY(ps.linear("time_embedding.linear_2", T, T, true, false, &t.te2));
    TRY(ps.linear("context_embedding.0", T, cross, true, false, &t.ce1));
    TRY(ps.linear("context_embedding.2", cross * ic, T, true, false, &t.ce2));
    TRY(ps.linear("fps_embedding.0", T, C0, true, false, &t.fe1));
    TRY(ps.linear("fps_embedding.2", T, T, true, false, &t.fe2));
    // down blocks; the skip channels in the order the reference collects them
    std::vector<int> skip_c = {C0};
    t.down.resize(nl);
    int cin = C0;
    for (int i = 0; i < nl; ++i) {
        IBlockW& d = t.down[i];
        const std::string pre = "down_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[i] != 0;
        const int n = c.layers_per_block;
        d.Cout = c.block_out_channels[i];
        d.res.resize(n); d.tconv.resize(n);
        if (attn) { d.attn.resize(n); d.tattn.resize(n); }
        for (int j = 0; j < n; ++j) {
            TRY(build_layer(ps, t, d, pre, j, j == 0 ? cin : d.Cout, attn));
            skip_c.push_back(d.Cout);
        }
        d.resample = i + 1 < nl;
        if (d.resample) {
            TRY(ps.conv(pre + ".downsamplers.0.conv", d.Cout, d.Cout, 3, false, &d.conv, /*split*/ true));
            skip_c.push_back(d.Cout);
        }
        cin = d.Cout;
    }
    // UNetMidBlock3DCrossAttn: resnets.0, temp_convs.0, attentions.0, temp_attentions.0, resnets.1, temp_convs.1
    {
        const int Cm = c.block_out_channels[nl - 1];
        IBlockW& m = t.mid;
        m.Cout = Cm;
        m.res.resize(2); m.tconv.resize(2); m.attn.resize(1); m.tattn.resize(1);
        TRY(build_layer(ps, t, m, "mid_block", 0, Cm, true));
        TRY(build_layer(ps, t, m, "mid_block", 1, Cm, false));
    }
    // up blocks: layers_per_block + 1 layers over [h | skip]
    t.up.resize(nl);
    int prev = c.block_out_channels[nl - 1];
    size_t si = skip_c.size();
    for (int i = 0; i < nl; ++i) {
        IBlockW& u = t.up[i];
        const int li = nl - 1 - i, n = c.layers_per_block + 1;
        const std::string pre = "up_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[li] != 0;
        u.Cout = c.block_out_channels[li];
        u.res.resize(n); u.tconv.resize(n);
        if (attn) { u.attn.resize(n); u.tattn.resize(n); }
        for (int j = 0; j < n; ++j) {
            const int cskip = skip_c[--si];
            TRY(build_layer(ps, t, u, pre, j, (j == 0 ? prev : u.Cout) + cskip, attn));
        }
        u.resample = i + 1 < nl;
        if (u.resample) TRY(ps.conv(pre + ".upsamplers.0.conv", u.Cout, u.Cout, 3, false, &u.conv, /*split*/ true));     // (no phase pack: the 9-tap gather)
        prev = u.Cout;
    }
    CTRL_CHECK(si == 0, "unet_i2v: skip bookkeeping");
    TRY(ps.norm("conv_norm_out", C0, &t.norm_out));
    TRY(ps.conv_direct("conv_out", c.out_channels, C0, &t.conv_out));
    TRY(ps.linear_cat(t.temb_names, t.temb_ns, T, true, &t.temb_cat));
    return 0;
}

// the latent encoder's eleven tensors as one block, in op_i2v_latent_encoder's order (they were requested in that order)
int pack_encoder(UNetI2V& t, hipStream_t s) {
    static const int n[11] = {4, 4, 32, 32, 32, 32, 4, 64, 16, 64, 4};
    TRY(t.pk->dalloc(kEncWts * sizeof(float), (void**)&t.enc_w));
    int off = 0;
    for (int i = 0; i < 11; ++i) {
        HIP_TRY(hipMemcpyAsync(t.enc_w + off, t.enc_part[i], n[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
        off += n[i];
    }
    CTRL_CHECK(off == kEncWts, "unet_i2v: latent encoder weight bookkeeping");
    return 0;
}

int collect(const ctrl_unet_i2v_config& c, SpecCollector& sc) {
    TRY(validate(c));
    UNetI2V t;
    t.cfg = c;
    return build_unet(sc, t);
}

struct UFwd {
    const void* sample; int dt; int B, F, h, w;
    const float* t; int t_count;
    const float* fps; int fps_count;
    const void* lat; int lat_dt;
    const void* emb; int emb_dt;
    const void* ehs; int ehs_dt, Lt;
    const void* const* down_res; int n_down_res, down_dt, down_5d;
    const void* mid_res; int mid_dt, mid_5d;
    void* out;
};

struct Pre {
    float* tproj = nullptr;                 // [B][temb_total]
    float* op8 = nullptr;                   // conv_in's operand rows [(b f) h w][8]
    std::vector<PreKV> kv;                  // one per cross-attention, in forward order
    size_t next = 0;
    EhsCtx e;
};

// everything that depends on (timestep, fps) and on the condition (text states, image latents, image embeddings) only
int precompute(Ctx& cx, UNetI2V& t, const UFwd& a, Pre* P) {
    const ctrl_unet_i2v_config& c = t.cfg;
    const int B = a.B, F = a.F, N = B * F, h = a.h, w = a.w, hw = h * w, C0 = c.block_out_channels[0], T = 4 * C0;
    const int cross = c.cross_attention_dim, ic = c.in_channels, Lk = a.Lt + kLatTokens + ic;
    const bool reuse = t.kvc.mode == KvCache::REUSE, keep = t.kvc.mode == KvCache::KEEP;
    std::vector<SmallLin> L1, L2;
    float* tsin = cx.f((size_t)B * C0); float* fsin = cx.f((size_t)B * C0);
    RUN(cx, op_timestep_sincos(a.t, a.t_count, tsin, B, C0, cx.s));
    RUN(cx, op_timestep_sincos(a.fps, a.fps_count, fsin, B, C0, cx.s));
    float* t1 = cx.f((size_t)B * T); float* f1 = cx.f((size_t)B * T);
    float* et = cx.f((size_t)B * T); float* ef = cx.f((size_t)B * T);
    L1.push_back({tsin, C0, t.te1.w, t.te1.b, t1, T, B, T, C0, 0, 1});
    L1.push_back({fsin, C0, t.fe1.w, t.fe1.b, f1, T, B, T, C0, 0, 1});
    L2.push_back({t1, T, t.te2.w, t.te2.b, et, T, B, T, T, 0, 0});
    L2.push_back({f1, T, t.fe2.w, t.fe2.b, ef, T, B, T, T, 0, 0});
    float* ci = nullptr;                    // context_embedding(image_embeddings) [B][ic * cross]
    if (!reuse) {
        float* e32 = cx.f((size_t)B * cross);
        float* c1 = cx.f((size_t)B * T);
        ci = cx.f((size_t)B * ic * cross);
        // (the frames kernel with one frame is the plain conversion to fp32: [1][4][1][B * cross / 4])
        RUN(cx, op_i2v_frames(a.emb, a.emb_dt, e32, 1, 1, B * cross / 4, cx.s));
        L1.push_back({e32, cross, t.ce1.w, t.ce1.b, c1, T, B, T, cross, 0, 1});
        L2.push_back({c1, T, t.ce2.w, t.ce2.b, ci, (long)ic * cross, B, ic * cross, T, 0, 0});
    }
    RUN(cx, op_linear_small_group(L1.data(), (int)L1.size(), cx.s));
    RUN(cx, op_linear_small_group(L2.data(), (int)L2.size(), cx.s));
    // emb = time_embedding + fps_embedding; every ResNet starts with SiLU(emb): applied on load by the batched projection
    float* emb = cx.f((size_t)B * T);
    RUN(cx, op_add_rowvec(et, DT_F32, ef, T, emb, DT_F32, (size_t)B, T, 1, B, cx.s));
    P->tproj = cx.f((size_t)B * t.temb_total);
    RUN(cx, op_linear_small(emb, T, t.temb_cat.w, t.temb_cat.b, P->tproj, t.temb_total, B, t.temb_total, T, 1, 0, cx.s));
    P->op8 = cx.f((size_t)N * hw * 8);
    P->e.batch = B; P->e.Lk = Lk; P->e.cross = cross;
    if (!reuse) {
        float* lat32 = cx.f((size_t)N * 4 * hw);                      // (b f) c h w planes
        RUN(cx, op_i2v_frames(a.lat, a.lat_dt, lat32, B, F, hw, cx.s));
        // ---- the context matrix [B][Lk][cross] in fp16: text | 64 latent tokens | ic image-embedding tokens ----
        half_t* ctx = cx.h((size_t)B * Lk * cross);
        half_t* c0 = cx.h((size_t)B * hw * 8 * ic);
        half_t* pool = cx.h((size_t)B * kPool * kPool * 8 * ic);
        half_t* c1 = cx.h((size_t)B * (kPool / 2) * (kPool / 2) * 16 * ic);
        for (int b = 0; b < B; ++b)       // frame 0 of every clip
            RUN(cx, op_conv3x3_direct(lat32 + (size_t)b * F * 4 * hw, DT_F32, 1, t.ctx0.w, t.ctx0.b, c0 + (size_t)b * hw * 8 * ic, 1, 4, 8 * ic, h, w, 1, 1, cx.s));
        RUN(cx, op_adaptive_avgpool_nhwc(c0, DT_F16, pool, DT_F16, B, h, w, 8 * ic, kPool, kPool, cx.s));
        ConvOpts o1; o1.stride = 2; o1.act = 1;
        TRY(run_conv(cx, t.ctx1, pool, tv16(c1), B, kPool, kPool, o1));
        const size_t esz = a.ehs_dt == DT_F32 ? 4 : 2;
        for (int b = 0; b < B; ++b) {
            half_t* rows = ctx + (size_t)b * Lk * cross;
            RUN(cx, op_nchw_to_nhwc((const char*)a.ehs + (size_t)b * a.Lt * cross * esz, a.ehs_dt, rows, 1, 1, a.Lt * cross, cx.s));
            ConvOpts o2; o2.stride = 2;
            TRY(run_conv(cx, t.ctx2, c1 + (size_t)b * (kPool / 2) * (kPool / 2) * 16 * ic, tv16(rows + (size_t)a.Lt * cross), 1, kPool / 2, kPool / 2, o2));
            RUN(cx, op_nchw_to_nhwc(ci + (size_t)b * ic * cross, DT_F32, rows + (size_t)(a.Lt + kLatTokens) * cross, 1, 1, ic * cross, cx.s));
        }
        P->e.h16 = ctx;
        // ---- image_latents_proj_in over every frame, then the temporal encoder beside the sample ----
        half_t* p0 = cx.h((size_t)N * hw * 4 * ic);
        half_t* p1 = cx.h((size_t)N * hw * 4 * ic);
        float* p2 = cx.f((size_t)N * hw * ic);
        RUN(cx, op_conv3x3_direct(lat32, DT_F32, 1, t.pi0.w, t.pi0.b, p0, N, 4, 4 * ic, h, w, 1, 1, cx.s));
        if (t.pi1.w16 && !policy_is0(P_SMALLCONV_MFMA)) RUN(cx, op_conv3x3_small_mfma(p0, t.pi1.w16, t.pi1.b, p1, N, 4 * ic, 4 * ic, h, w, 1, 1, cx.s));
        else RUN(cx, op_conv3x3_direct(p0, DT_F16, 0, t.pi1.w, t.pi1.b, p1, N, 4 * ic, 4 * ic, h, w, 1, 1, cx.s));
        RUN(cx, op_unet_conv_out(p1, t.pi2.w, t.pi2.b, p2, DT_F32, N, h, w, 4 * ic, ic, cx.s, CONV_OUT_ROWS));
        RUN(cx, op_i2v_latent_encoder(p2, t.enc_w, a.sample, a.dt, P->op8, keep ? t.lat_keep : nullptr, B, F, hw, 0, cx.s));
    } else {
        RUN(cx, op_i2v_latent_encoder(t.lat_keep, nullptr, a.sample, a.dt, P->op8, nullptr, B, F, hw, 1, cx.s));
    }
    // K / V^T of the context for every cross-attention of the forward, in forward order (kept / reused through the plan's cache)
    std::vector<const BasicTBW*> tbs;
    for (const IBlockW& d : t.down) for (const STfmW& s : d.attn) tbs.push_back(&s.tb);
    for (const STfmW& s : t.mid.attn) tbs.push_back(&s.tb);
    for (const IBlockW& u : t.up) for (const STfmW& s : u.attn) tbs.push_back(&s.tb);
    P->kv.assign(tbs.size(), PreKV());
    // (uncached, the projections live in the workspace behind the stems' scratch for the whole forward: a few MB, not given back)
    for (size_t i = 0; i < tbs.size(); ++i) TRY(project_text_kv(cx, tbs[i]->attn2, P->e, &P->kv[i]));
    return 0;
}

// fp32 stream [rows][C]; its fp16 mirror, where a main-path convolution reads it, is a split [hi | lo] row pair, 2 C wide
TV stream_f32(Ctx& cx, size_t rows, int C, bool need16) {
    TV t;
    t.p = cx.f(rows * C); t.dt = DT_F32;
    if (need16) { t.m16 = cx.h(rows * C * 2); t.lo_off = C; }
    return t;
}

// out (row stride ldo) = TemporalConvLayer(x) over B clips of F frames with HW pixels; x dense [M][C]
int run_temporal_conv(Ctx& cx, const TConvW& w, const TV& x, const TV& out, long ldo, int B, int F, int HW) {
    const int C = w.c[0].Cout, M = B * F * HW;
    const size_t mk = cx.mark();
    const bool sd = w.c[0].dup;                       // split operand: rows [hi | lo], the weights packed twice
    const int K = w.c[0].Cin;                         // C, or 2 C
    half_t* n1 = cx.h((size_t)M * K);
    TV ping = stream_alloc(cx, (size_t)M * C, false), pong = stream_alloc(cx, (size_t)M * C, false);
    TV cur = x;
    for (int i = 0; i < 4; ++i) {
        TRY(run_groupnorm(cx, w.n[i], cur, n1, B, F * HW, 1e-5f, true, sd));      // statistics span the clip's frames
        IGemmArgs g = {};
        g.A = n1; g.lda = K; g.mode = IG_TEMPORAL; g.Cin = K; g.taps = 3; g.F = F; g.HW = HW; g.t_pad = 0; g.a_split = sd ? 1 : 0;
        g.W = w.c[i].w; g.M = M; g.Nout = C; g.Ktot = 3 * K; g.bias = w.c[i].b; g.rows_per_img = HW; g.scale = 1.f;
        if (i < 3) {
            const TV dst = (i & 1) ? pong : ping;
            set_out(g, dst, C, C);
            RUN(cx, op_igemm(g, cx.s));
            cur = dst;
        } else {
            set_res(g, x, C);                         // identity + conv4(...)
            set_out(g, out, ldo, C);
            RUN(cx, op_igemm(g, cx.s));
        }
    }
    cx.release(mk);
    return 0;
}

// out (row stride ldo) = TransformerTemporalModel(x); x dense [M][C], rows (b, f, p)
int run_temporal_tfm(Ctx& cx, const TTfmW& w, const TV& x, const TV& out, long ldo, int B, int F, int HW) {
    const int C = w.C, Ci = w.inner, M = B * F * HW;
    const size_t mk = cx.mark();
    half_t* n = cx.h((size_t)M * C);
    TRY(run_groupnorm(cx, w.norm, x, n, B, F * HW, 1e-6f, false));                 // b c f h w statistics, no activation
    TV tok = stream_alloc(cx, (size_t)M * Ci, false);
    half_t* xn = cx.h((size_t)M * Ci);
    TRY(run_linear(cx, w.proj_in, n, C, tok, Ci, M, TV(), 0, nullptr, 0, 0, nullptr, TV(), &w.ln1, xn));
    half_t* qkv = cx.h((size_t)M * 3 * Ci);
    half_t* o = cx.h((size_t)M * Ci);
    TV x1 = stream_alloc(cx, (size_t)M * Ci, false), x2 = stream_alloc(cx, (size_t)M * Ci, false);
    const AttnW* at[2] = {&w.a1, &w.a2};
    const Norm* ln_next[2] = {&w.ln2, &w.ln3};
    TV src = tok;
    for (int k = 0; k < 2; ++k) {
        const TV dst = k == 0 ? x1 : x2;
        TRY(run_linear(cx, at[k]->qkv, xn, Ci, tv16(qkv), 3 * Ci, M, TV(), 0));
        TAttnArgs ta = {};
        ta.Q = qkv; ta.ld = 3 * Ci; ta.O = o; ta.ldo = Ci; ta.Bc = B; ta.F = F; ta.HW = HW; ta.heads = at[k]->heads;
        ta.scale = 0.125f;
        RUN(cx, op_temporal_attn(ta, cx.s));
        TRY(run_linear(cx, at[k]->out, o, Ci, dst, Ci, M, src, Ci, nullptr, 0, 0, nullptr, TV(), ln_next[k], xn));
        src = dst;
    }
    // behind the feed-forward the tokens are proj_out's operand only: fp16
    TV x3 = tv16(cx.h((size_t)M * Ci));
    TRY(run_ffn(cx, w.ff1, w.ff2, xn, Ci, x3, M, x2));
    TRY(run_linear(cx, w.proj_out, x3.m16, Ci, out, ldo, M, x, C));
    cx.release(mk);
    return 0;
}

// out (row stride ldo) = Transformer2DModel(x) over N = B * F images of L pixels; the cross-attention as B problems of F * L queries
int run_spatial_tfm(Ctx& cx, const STfmW& w, const TV& x, const TV& out, long ldo, int B, int F, int L, Pre& P) {
    const int N = B * F, M = N * L, C = w.C;
    const size_t mk = cx.mark();
    half_t* n = cx.h((size_t)M * C);
    TRY(run_groupnorm(cx, w.norm, x, n, N, L, 1e-6f, false));
    TV tok = stream_alloc(cx, (size_t)M * C, false);
    half_t* tok_ln = cx.h((size_t)M * C);
    TRY(run_linear(cx, w.proj_in, n, C, tok, C, M, TV(), 0, nullptr, 0, 0, nullptr, TV(), &w.tb.norm1, tok_ln));
    TV t2 = tv16(cx.h((size_t)M * C));          // proj_out's operand only: fp16
    CTRL_CHECK(P.next < P.kv.size(), "unet_i2v: cross-attention bookkeeping");
    const PreKV* kv = &P.kv[P.next++];
    TRY(run_basic_tb(cx, w.tb, tok, t2, N, L, P.e, nullptr, kv, tok_ln, 0, /*cross_B*/ B));
    TRY(run_linear(cx, w.proj_out, t2.m16, C, out, ldo, M, x, C));
    cx.release(mk);
    return 0;
}

// layer j of a block: x (dense [M][Cin], or the concatenated operand) -> dst (row stride ldd)
int run_layer(Ctx& cx, const UNetI2V& t, const IBlockW& b, int j, bool attn, const TV& x, const TV& dst, long ldd, const UFwd& a, int h, int w,
              Pre& P) {
    const int B = a.B, F = a.F, N = B * F, HW = h * w, C = b.Cout;
    const size_t rows = (size_t)N * HW;
    const size_t mk = cx.mark();
    TV r = stream_f32(cx, rows, C, false);
    TRY(run_resnet(cx, b.res[j].r, x, r, N, h, w, 1, P.tproj + b.res[j].toff, t.temb_total, 1e-5f, 0, F * HW));
    if (!attn) {
        TRY(run_temporal_conv(cx, b.tconv[j], r, dst, ldd, B, F, HW));
    } else {
        TV tc = stream_f32(cx, rows, C, false), sa = stream_f32(cx, rows, C, false);
        TRY(run_temporal_conv(cx, b.tconv[j], r, tc, C, B, F, HW));
        TRY(run_spatial_tfm(cx, b.attn[j], tc, sa, C, B, F, HW, P));
        TRY(run_temporal_tfm(cx, b.tattn[j], sa, dst, ldd, B, F, HW));
    }
    cx.release(mk);
    return 0;
}

struct Skip { TV x; int C, h, w; };

int unet_run(Ctx& cx, UNetI2V& t, const UFwd& a) {
    const ctrl_unet_i2v_config& c = t.cfg;
    const int nl = c.num_levels, B = a.B, F = a.F, N = B * F, C0 = c.block_out_channels[0];
    cx.stats_off = 0;
    t.kvc.next = 0;
    TRY(begin_forward(cx));
    Pre P;
    TRY(precompute(cx, t, a, &P));
    // ---- conv_in over [sample | encoded latents], then transformer_in: skip 0 ----
    int h = a.h, w = a.w;
    std::vector<Skip> skips;
    TV cur = stream_f32(cx, (size_t)N * h * w, C0, false);
    {
        const size_t mk = cx.mark();
        TV ci = stream_f32(cx, (size_t)N * h * w, C0, false);
        RUN(cx, op_conv3x3_rows_f32(P.op8, t.conv_in.w, t.conv_in.b, (float*)ci.p, N, 2 * c.in_channels, C0, h, w, cx.s));
        TRY(run_temporal_tfm(cx, t.tin, ci, cur, C0, B, F, h * w));
        cx.release(mk);
    }
    skips.push_back({cur, C0, h, w});
    // ---- down blocks ----
    for (int i = 0; i < nl; ++i) {
        const IBlockW& d = t.down[i];
        const int C = d.Cout, nres = (int)d.res.size();
        for (int j = 0; j < nres; ++j) {
            const bool to_conv = j + 1 == nres && d.resample;         // the down-sampler reads the fp16 mirror
            TV y = stream_f32(cx, (size_t)N * h * w, C, to_conv);
            TRY(run_layer(cx, t, d, j, !d.attn.empty(), cur, y, C, a, h, w, P));
            cur = y;
            skips.push_back({cur, C, h, w});
        }
        if (d.resample) {
            const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
            TV y = stream_f32(cx, (size_t)N * ho * wo, C, t.down[i + 1].res[0].r.has_shortcut);
            ConvOpts o; o.stride = 2;
            TRY(run_conv(cx, d.conv, cur.m16, y, N, h, w, o));
            cur = y; h = ho; w = wo;
            skips.push_back({cur, C, h, w});
        }
    }
    // ---- mid block; its output is the h half of the first up layer's operand ----
    size_t si = skips.size();
    auto alloc_cat = [&](size_t rows, int C1) { return stream_f32(cx, rows, C1 + skips[si - 1].C, true); };
    const int Cm = t.mid.Cout;
    TV cat = alloc_cat((size_t)N * h * w, Cm);
    int C1 = Cm;
    {
        const size_t mk = cx.mark();
        TV m0 = stream_f32(cx, (size_t)N * h * w, Cm, false);
        TRY(run_layer(cx, t, t.mid, 0, true, cur, m0, Cm, a, h, w, P));
        TRY(run_layer(cx, t, t.mid, 1, false, m0, cat, Cm + skips[si - 1].C, a, h, w, P));
        cx.release(mk);
    }
    if (a.mid_res)      // :710-713, in place over the mid stream
        RUN(cx, op_unet_skip_join((const float*)cat.p, Cm + skips[si - 1].C, a.mid_res, a.mid_dt, a.mid_5d, B, F, h * w, Cm, (float*)cat.p,
                                  cat.m16, Cm + skips[si - 1].C, 0, cx.s, cat.lo_off));
    // ---- up blocks ----
    TV fin;
    for (int i = 0; i < nl; ++i) {
        const IBlockW& u = t.up[i];
        const int C = u.Cout, nres = (int)u.res.size();
        for (int j = 0; j < nres; ++j) {
            CTRL_CHECK(si >= 1, "unet_i2v: skip bookkeeping");
            const Skip& sk = skips[--si];
            CTRL_CHECK(sk.h == h && sk.w == w && C1 + sk.C == u.res[j].r.Cin, "unet_i2v: skip shape bookkeeping");
            const int Ct = C1 + sk.C;
            const void* res = (int)si < a.n_down_res ? a.down_res[si] : nullptr;       // zip(): skip i takes residual i
            RUN(cx, op_unet_skip_join((const float*)sk.x.p, sk.C, res, a.down_dt, a.down_5d, B, F, h * w, sk.C, (float*)cat.p, cat.m16, Ct, C1, cx.s, cat.lo_off));
            const size_t rows = (size_t)N * h * w;
            const bool last = j + 1 == nres;
            // where this layer's output goes: the h half of the next operand, the up-sampler's operand, or the head
            TV dst; long ldd = C;
            if (!last) { dst = alloc_cat(rows, C); ldd = C + skips[si - 1].C; }
            else dst = stream_f32(cx, rows, C, u.resample);
            TRY(run_layer(cx, t, u, j, !u.attn.empty(), cat, dst, ldd, a, h, w, P));
            if (!last) { cat = dst; C1 = C; }
            else fin = dst;
        }
        if (u.resample) {
            cat = alloc_cat((size_t)N * 4 * h * w, C);
            ConvOpts o; o.up = 2; o.ldy = C + skips[si - 1].C;
            TRY(run_conv(cx, u.conv, fin.m16, cat, N, h, w, o));
            h *= 2; w *= 2; C1 = C;
        }
    }
    CTRL_CHECK(si == 0 && h == a.h && w == a.w && P.next == P.kv.size(), "unet_i2v: skip / cross-attention bookkeeping");
    // ---- conv_norm_out + SiLU + conv_out -> b c f h w in the sample's dtype ----
    half_t* nf = cx.h((size_t)N * h * w * C0);
    TRY(run_groupnorm(cx, t.norm_out, fin, nf, N, h * w, 1e-5f, true));
    RUN(cx, op_unet_conv_out(nf, t.conv_out.w, t.conv_out.b, a.out, a.dt, N, h, w, C0, c.out_channels, cx.s, CONV_OUT_NCFHW, F));
    return 0;
}

bool dt_ok(int dt) { return dt == DT_F32 || dt == DT_F16 || dt == DT_BF16; }

int forward(UNetI2V& t, const UFwd& a, hipStream_t s) {
    const ctrl_unet_i2v_config& c = t.cfg;
    CTRL_CHECK(a.sample && a.t && a.fps && a.lat && a.emb && a.ehs && a.out, "unet_i2v_forward: null argument");
    CTRL_CHECK(dt_ok(a.dt) && dt_ok(a.lat_dt) && dt_ok(a.emb_dt) && dt_ok(a.ehs_dt),
               "unet_i2v_forward: sample, image_latents, image_embeddings and encoder_hidden_states must be fp32, fp16 or bf16");
    CTRL_CHECK(a.B >= 1 && a.B <= 64 && a.F >= 1 && a.F <= 32, "unet_i2v_forward: 1 .. 64 clips of 1 .. 32 frames (the temporal attention's limit)");
    CTRL_CHECK(a.Lt >= 1 && a.Lt <= 4096, "unet_i2v_forward: 1 .. 4096 text tokens");
    const int m = 1 << (c.num_levels - 1);
    CTRL_CHECK(a.h >= m && a.w >= m && a.h % m == 0 && a.w % m == 0, "unet_i2v_forward: the latent height and width must be multiples of 2^(levels - 1)");
    CTRL_CHECK((double)a.B * a.F * a.h * a.w * 2.0 * c.block_out_channels[0] < 2147483648.0,
               "unet_i2v_forward: the clip batch is too large (frames x pixels x concatenated channels must stay below 2^31 elements)");
    CTRL_CHECK(a.t_count == 1 || a.t_count == a.B, "unet_i2v_forward: need 1 or B timesteps");
    CTRL_CHECK(a.fps_count == 1 || a.fps_count == a.B, "unet_i2v_forward: need 1 or B fps values");
    CTRL_CHECK(a.n_down_res >= 0 && (a.n_down_res == 0 || a.down_res), "unet_i2v_forward: bad residual list");
    for (int i = 0; i < a.n_down_res; ++i) CTRL_CHECK(a.down_res[i] != nullptr, "unet_i2v_forward: null residual");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    const int key[5] = {a.B, a.F, a.h, a.w, a.Lt};
    if (t.kvc.mode == KvCache::KEEP) {
        const size_t need = (size_t)a.B * a.F * a.h * a.w * 4;
        CTRL_CHECK(!(capturing && (t.kvc.slots.empty() || t.lat_elems < need)),
                   "condition cache: the first KEEP forward of a shape allocates its buffers and cannot run under stream capture -- run it eagerly once, then capture");
        if (t.lat_elems < need) {
            if (t.lat_keep) t.lat_retired.push_back(t.lat_keep);       // captured graphs may still address it
            t.lat_keep = nullptr; t.lat_elems = 0;
            HIP_TRY(hipMalloc((void**)&t.lat_keep, need * sizeof(float)));
            t.lat_elems = need;
        }
    }
    if (t.kvc.mode == KvCache::REUSE) {
        bool same = t.lat_keep != nullptr;
        for (int i = 0; i < 5; ++i) same = same && t.key[i] == key[i];
        CTRL_CHECK(same, "unet_i2v_forward: condition cache REUSE without a KEEP forward of this batch, clip length, latent size and prompt length");
    }
    t.ar.off = 0; t.ar.peak = 0;
    Ctx dry{&t.ar, s, true};
    dry.kvc = &t.kvc;
    TRY(unet_run(dry, t, a));
    TRY(t.reserve(workspace_bytes(dry), capturing, "unet_i2v", "size"));
    t.ar.off = 0;
    Ctx cx{&t.ar, s, false};
    cx.kvc = &t.kvc;
    cx.capturing = capturing;
    cx.stats_total = dry.stats_total;
    TRY(unet_run(cx, t, a));
    if (t.kvc.mode == KvCache::KEEP) for (int i = 0; i < 5; ++i) t.key[i] = key[i];
    return t.leave(s, capturing);
}

}  // namespace

extern "C" {

int ctrl_unet_i2v_param_count(const ctrl_unet_i2v_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_unet_i2v_param_spec(const ctrl_unet_i2v_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "unet_i2v_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "unet_i2v_param_spec", name, name_len, shape, ndim);
}

int ctrl_unet_i2v_create(const ctrl_unet_i2v_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet_i2v** out) {
    return plan_create<UNetI2V>("unet_i2v_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_unet, pack_encoder);
}

void ctrl_unet_i2v_destroy(ctrl_unet_i2v* h) { plan_destroy<UNetI2V>(h); }

int ctrl_unet_i2v_selection(ctrl_unet_i2v* h, char* buf, int len) {
    CTRL_CHECK(h && buf && len > 0, "unet_i2v_selection: null argument");
    const UNetI2V* t = (const UNetI2V*)h;
    snprintf(buf, (size_t)len, "streams=fp32 main_path_split_operands=1 resnet_split_operands=%d upsampler=gather9 cross_attentions=%d "
                               "cross_attention_problems=batch time_projection_columns=%d selection=default",
             t->split ? 1 : 0, t->n_cross, t->temb_total);
    return 0;
}

int ctrl_unet_i2v_set_cond_cache(ctrl_unet_i2v* h, int mode) {
    CTRL_CHECK(h && mode >= 0 && mode <= 2, "unet_i2v_set_cond_cache: mode must be 0 (off), 1 (keep) or 2 (reuse)");
    ((UNetI2V*)h)->kvc.mode = mode;
    return 0;
}

int64_t ctrl_unet_i2v_workspace_bytes(ctrl_unet_i2v* h) { return h ? (int64_t)((UNetI2V*)h)->ar.cap : -1; }

int ctrl_unet_i2v_forward(ctrl_unet_i2v* h, const void* sample, int sample_dtype, int B, int F, int lat_h, int lat_w, const float* timesteps,
                          int t_count, const float* fps, int fps_count, const void* image_latents, int latents_dtype,
                          const void* image_embeddings, int embeddings_dtype, const void* encoder_hidden_states, int ehs_dtype, int text_len,
                          const void* const* down_residuals, int n_down_residuals, int down_dtype, int down_5d, const void* mid_residual,
                          int mid_dtype, int mid_5d, void* out, void* stream) {
    CTRL_CHECK(h != nullptr, "unet_i2v_forward: null plan");
    UNetI2V* t = (UNetI2V*)h;
    DeviceGuard dg(t->device);
    const UFwd a = {sample, sample_dtype, B, F, lat_h, lat_w, timesteps, t_count, fps, fps_count, image_latents, latents_dtype,
                    image_embeddings, embeddings_dtype, encoder_hidden_states, ehs_dtype, text_len,
                    down_residuals, n_down_residuals, down_dtype, down_5d, mid_residual, mid_dtype, mid_5d, out};
    return forward(*t, a, S(stream));
}

int ctrl_op_i2v_latent_encoder(const float* x, const float* weights, const void* sample, int sample_dtype, float* out8, float* keep, int B,
                               int F, int HW, int precomputed, void* stream) {
    return op_i2v_latent_encoder(x, weights, sample, sample_dtype, out8, keep, B, F, HW, precomputed, S(stream));
}

int ctrl_op_adaptive_avgpool_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int N, int H, int W, int C, int OH, int OW, void* stream) {
    return op_adaptive_avgpool_nhwc(x, x_dtype, y, y_dtype, N, H, W, C, OH, OW, S(stream));
}

}  // extern "C"
