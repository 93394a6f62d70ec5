// SVD backbone UNet plan (diffusers v0.27 UNetSpatioTemporalConditionModel as the reference extends it with the two ControlNet residual
// kwargs: svd/models/unets/unet_spatio_temporal_condition.py, constructor :70-246, forward :357-526).  Order of operations:
//   time_proj -> time_embedding, added_time_ids -> add_time_proj -> add_embedding, summed :389-420 | every ResNet's time projection,
//   spatial and temporal, as ONE small-M linear over the per-clip embedding (broadcast over the clip's frames by the convolutions'
//   rowvec with rows_per_img = F * H * W, never copied) | conv_in :432 | down blocks collecting the skips :438-454 | mid block :477 |
//   the residuals :457-490 | up blocks :495-513 | conv_norm_out + SiLU + conv_out :516-518, NCHW in the sample's dtype.
// Blocks (diffusers unet_3d_blocks.py): SpatioTemporalResBlock = run_resnet + a TemporalResnetBlock whose last Conv3d carries the fp32
// residual and the AlphaBlender fold (alpha * spatial + (1 - alpha) * temporal, alpha = sigmoid(mix_factor): set_blend's own
// orientation; image_only_indicator is all zero); TransformerSpatioTemporalModel = GroupNorm, proj_in, per layer BasicTransformerBlock,
// + frame-index embedding, TemporalBasicTransformerBlock, AlphaBlender, then proj_out + input.  encoder_hidden_states hold ONE key, so
// both cross-attentions are a vector per clip (SURVEY.md note N5); the temporal one pairs row (b L + p) with clip (b L + p) % B, the
// reference's time_context broadcast (op_add_rowvec_clip).
// Activations are frame-major channels-last [(b f) h w][C]; residual streams fp32, fp16 mirrors where a GEMM reads them.  The up path
// never concatenates: the operand [rows][C1 + C2] of an up ResNet is allocated first, the producer of its h half writes columns
// [0, C1) through the output row stride, op_unet_skip_join writes the skip (+ the adapter's residual) into columns [C1, C1 + C2).
// One stream, no lanes, no grouped launches: capturable as a linear graph.
#include "plan_common.h"
#include <cstdio>

namespace {

struct USTResW {                 // SpatioTemporalResBlock with time embeddings
    ResnetW sp;                  // spatial_res_block
    Norm tn1, tn2;               // temporal_res_block (C -> C)
    ConvW tc1, tc2;
    int toff_s = 0, toff_t = 0;  // columns of the two time_emb_proj inside the batched projection
    float* mix = nullptr;
    float eps = 1e-6f;
};

struct UTfmW {                   // TransformerSpatioTemporalModel
    Norm norm;
    Lin proj_in, proj_out, tpe1, tpe2;
    std::vector<BasicTBW> tb;
    std::vector<TemporalTBW> ttb;
    float* mix = nullptr;
    int C = 0;
};

struct UBlockW {
    std::vector<USTResW> res;
    std::vector<UTfmW> attn;     // empty: a block without attention
    bool resample = false;
    ConvW conv;                  // downsamplers.0.conv | upsamplers.0.conv
    int Cout = 0;
};

struct UNetST : StandalonePlan {
    ctrl_unet_st_config cfg{};
    ConvD conv_in, conv_out;
    Lin te1, te2, ae1, ae2, temb_cat;
    std::vector<UBlockW> down, up;
    UBlockW mid;
    Norm norm_out;
    int temb_total = 0;
    // split [hi | lo] operands for the 3x3 and the temporal convolutions of every ResNet (CTRL_UNET_SPLIT=1, read at plan creation): their
    // operand is a GroupNorm output, exact to ~2^-22 instead of 2^-11 at twice the matrix work of those launches.  Off by default: measured
    // on the narrow test configs it does not move the output error, which the fp16 token operands of the transformers set
    bool split = false;
    std::vector<std::string> temb_names;
    std::vector<int> temb_ns;
};

int validate(const ctrl_unet_st_config& c) {
    CTRL_CHECK(c.num_levels >= 1 && c.num_levels <= 4, "unet_st: 1 .. 4 levels");
    CTRL_CHECK(c.in_channels == 8, "unet_st: in_channels must be 8 (the stem kernel's instantiation)");
    CTRL_CHECK(c.out_channels >= 1 && c.out_channels <= 4, "unet_st: out_channels must be 1 .. 4");
    CTRL_CHECK(c.layers_per_block >= 1 && c.layers_per_block <= 4, "unet_st: layers_per_block out of range");
    CTRL_CHECK(c.transformer_layers_per_block >= 1 && c.transformer_layers_per_block <= 4, "unet_st: transformer_layers_per_block out of range");
    for (int i = 0; i < c.num_levels; ++i) {
        const int C = c.block_out_channels[i];
        CTRL_CHECK(C >= 64 && C % 64 == 0 && C <= 2048, "unet_st: block_out_channels must be multiples of 64 up to 2048");
        CTRL_CHECK((!c.level_has_attn[i] && i + 1 < c.num_levels) || (c.num_attention_heads[i] >= 1 && C == 64 * c.num_attention_heads[i]),
                   "unet_st: attention_head_dim (out_channels / heads) must be 64 at every attention level and in the mid block");
    }
    CTRL_CHECK(c.cross_attention_dim >= 8 && c.cross_attention_dim % 8 == 0, "unet_st: cross_attention_dim must be a multiple of 8");
    CTRL_CHECK(c.addition_time_embed_dim >= 8 && c.addition_time_embed_dim % 8 == 0 &&
                   c.projection_class_embeddings_input_dim % c.addition_time_embed_dim == 0 && c.projection_class_embeddings_input_dim >= c.addition_time_embed_dim,
               "unet_st: projection_class_embeddings_input_dim must be a multiple of addition_time_embed_dim (a multiple of 8)");
    return 0;
}

int build_st_res(ParamSink& ps, UNetST& t, const std::string& pre, int Cin, int Cout, float eps, USTResW* w) {
    TRY(build_resnet(ps, pre + ".spatial_res_block", Cin, Cout, false, &w->sp, t.split, /*shortcut: plain, it reads the stream's mirror*/ 0));
    const std::string tp = pre + ".temporal_res_block";
    TRY(ps.norm(tp + ".norm1", Cout, &w->tn1));
    TRY(ps.conv(tp + ".conv1", Cout, Cout, 3, /*temporal*/ true, &w->tc1, t.split));
    TRY(ps.norm(tp + ".norm2", Cout, &w->tn2));
    TRY(ps.conv(tp + ".conv2", Cout, Cout, 3, true, &w->tc2, t.split));
    TRY(ps.scalar(pre + ".time_mixer.mix_factor", &w->mix));
    w->eps = eps;
    w->toff_s = t.temb_total; t.temb_total += Cout;
    t.temb_names.push_back(pre + ".spatial_res_block.time_emb_proj"); t.temb_ns.push_back(Cout);
    w->toff_t = t.temb_total; t.temb_total += Cout;
    t.temb_names.push_back(tp + ".time_emb_proj"); t.temb_ns.push_back(Cout);
    return 0;
}

int build_tfm(ParamSink& ps, const ctrl_unet_st_config& c, const std::string& pre, int C, int heads, UTfmW* w) {
    w->C = C;
    TRY(ps.norm(pre + ".norm", C, &w->norm));
    TRY(ps.linear(pre + ".proj_in", C, C, true, false, &w->proj_in));
    w->tb.resize(c.transformer_layers_per_block);
    w->ttb.resize(c.transformer_layers_per_block);
    for (int k = 0; k < c.transformer_layers_per_block; ++k) {
        TRY(build_basic_tb(ps, pre + ".transformer_blocks." + std::to_string(k), C, heads, 64, c.cross_attention_dim, &w->tb[k]));
        TRY(build_temporal_tb(ps, pre + ".temporal_transformer_blocks." + std::to_string(k), C, heads, 64, c.cross_attention_dim, &w->ttb[k]));
    }
    TRY(ps.linear(pre + ".time_pos_embed.linear_1", 4 * C, C, true, false, &w->tpe1));
    TRY(ps.linear(pre + ".time_pos_embed.linear_2", C, 4 * C, true, false, &w->tpe2));
    TRY(ps.scalar(pre + ".time_mixer.mix_factor", &w->mix));
    TRY(ps.linear(pre + ".proj_out", C, C, true, false, &w->proj_out));
    return 0;
}

int build_unet(ParamSink& ps, UNetST& t) {
    const ctrl_unet_st_config& c = t.cfg;
    const int nl = c.num_levels, C0 = c.block_out_channels[0], T = 4 * C0;
    t.temb_total = 0; t.temb_names.clear(); t.temb_ns.clear();
    t.split = policy_is1(P_UNET_SPLIT);
    TRY(ps.conv_direct("conv_in", C0, c.in_channels, &t.conv_in));
    TRY(ps.linear("time_embedding.linear_1", T, C0, true, false, &t.te1));
    TRY(ps.linear("time_embedding.linear_2", T, T, true, false, &t.te2));
    TRY(ps.linear("add_embedding.linear_1", T, c.projection_class_embeddings_input_dim, true, false, &t.ae1));
    TRY(ps.linear("add_embedding.linear_2", T, T, true, false, &t.ae2));
    // down blocks; the skip channels in the order the reference collects them
    std::vector<int> skip_c = {C0};
    t.down.resize(nl);
    int cin = C0;
    for (int i = 0; i < nl; ++i) {
        UBlockW& d = t.down[i];
        const std::string pre = "down_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[i] != 0;
        d.Cout = c.block_out_channels[i];
        d.res.resize(c.layers_per_block);
        if (attn) d.attn.resize(c.layers_per_block);
        for (int j = 0; j < c.layers_per_block; ++j) {
            // CrossAttnDownBlockSpatioTemporal builds its ResNets with eps 1e-6, DownBlockSpatioTemporal with 1e-5
            TRY(build_st_res(ps, t, pre + ".resnets." + std::to_string(j), j == 0 ? cin : d.Cout, d.Cout, attn ? 1e-6f : 1e-5f, &d.res[j]));
            if (attn) TRY(build_tfm(ps, c, pre + ".attentions." + std::to_string(j), d.Cout, c.num_attention_heads[i], &d.attn[j]));
            skip_c.push_back(d.Cout);
        }
        d.resample = i + 1 < nl;
        if (d.resample) {
            TRY(ps.conv(pre + ".downsamplers.0.conv", d.Cout, d.Cout, 3, false, &d.conv));
            skip_c.push_back(d.Cout);
        }
        cin = d.Cout;
    }
    // UNetMidBlockSpatioTemporal: ResNet, transformer, ResNet (eps 1e-5)
    {
        const int Cm = c.block_out_channels[nl - 1];
        t.mid.Cout = Cm;
        t.mid.res.resize(2);
        t.mid.attn.resize(1);
        TRY(build_st_res(ps, t, "mid_block.resnets.0", Cm, Cm, 1e-5f, &t.mid.res[0]));
        TRY(build_tfm(ps, c, "mid_block.attentions.0", Cm, c.num_attention_heads[nl - 1], &t.mid.attn[0]));
        TRY(build_st_res(ps, t, "mid_block.resnets.1", Cm, Cm, 1e-5f, &t.mid.res[1]));
    }
    // up blocks: layers_per_block + 1 ResNets over [h | skip] (eps 1e-6)
    t.up.resize(nl);
    int prev = c.block_out_channels[nl - 1];
    size_t si = skip_c.size();
    for (int i = 0; i < nl; ++i) {
        UBlockW& u = t.up[i];
        const int li = nl - 1 - i;
        const std::string pre = "up_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[li] != 0;
        u.Cout = c.block_out_channels[li];
        u.res.resize(c.layers_per_block + 1);
        if (attn) u.attn.resize(c.layers_per_block + 1);
        for (int j = 0; j <= c.layers_per_block; ++j) {
            const int cskip = skip_c[--si];
            TRY(build_st_res(ps, t, pre + ".resnets." + std::to_string(j), (j == 0 ? prev : u.Cout) + cskip, u.Cout, 1e-6f, &u.res[j]));
            if (attn) TRY(build_tfm(ps, c, pre + ".attentions." + std::to_string(j), u.Cout, c.num_attention_heads[li], &u.attn[j]));
        }
        u.resample = i + 1 < nl;
        // (the up-sampler's 3x3 conv runs behind the nearest x2: it also gets the phase pack, four 2x2 convs over the source map)
        if (u.resample) TRY(ps.conv(pre + ".upsamplers.0.conv", u.Cout, u.Cout, 3, false, &u.conv, false, true));
        prev = u.Cout;
    }
    CTRL_CHECK(si == 0, "unet_st: skip bookkeeping");
    TRY(ps.norm("conv_norm_out", C0, &t.norm_out));
    TRY(ps.conv_direct("conv_out", c.out_channels, C0, &t.conv_out));
    TRY(ps.linear_cat(t.temb_names, t.temb_ns, T, true, &t.temb_cat));
    return 0;
}

int collect(const ctrl_unet_st_config& c, SpecCollector& sc) {
    TRY(validate(c));
    UNetST t;
    t.cfg = c;
    return build_unet(sc, t);
}

struct UFwd {
    const void* sample; int dt; int B, F, h, w;
    const float* t; int t_count;
    const void* ehs; int ehs_dt;
    const float* add_ids; int n_ids;
    const void* const* down_res; int n_down_res, down_dt, down_5d;
    const void* mid_res; int mid_dt, mid_5d;
    void* out;
};

struct TfmPre { const float* femb = nullptr; std::vector<const float*> s_ov, t_ov; };
struct Pre {
    float* tproj = nullptr;                 // [B][temb_total]
    std::vector<TfmPre> tf;                 // in forward order
    size_t next = 0;
    EhsCtx e;
};

// everything that depends on (timestep, added_time_ids, encoder_hidden_states, frame index) only: three levels of grouped small-M linears
int precompute(Ctx& cx, const UNetST& t, const UFwd& a, Pre* P) {
    const ctrl_unet_st_config& c = t.cfg;
    const int B = a.B, F = a.F, C0 = c.block_out_channels[0], T = 4 * C0, cross = c.cross_attention_dim;
    const int AD = c.addition_time_embed_dim, PD = c.projection_class_embeddings_input_dim;
    std::vector<SmallLin> L1, L2;
    float* tsin = cx.f((size_t)B * C0);
    RUN(cx, op_timestep_sincos(a.t, a.t_count, tsin, B, C0, cx.s));
    float* asin = cx.f((size_t)B * PD);                 // [B * n_ids][AD] == [B][PD]
    RUN(cx, op_timestep_sincos(a.add_ids, B * a.n_ids, asin, B * a.n_ids, AD, cx.s));
    float* t1 = cx.f((size_t)B * T); float* a1 = cx.f((size_t)B * T);
    float* et = cx.f((size_t)B * T); float* ea = cx.f((size_t)B * T);
    L1.push_back({tsin, C0, t.te1.w, t.te1.b, t1, T, B, T, C0, 0, 1});
    L1.push_back({asin, PD, t.ae1.w, t.ae1.b, a1, T, B, T, PD, 0, 1});
    L2.push_back({t1, T, t.te2.w, t.te2.b, et, T, B, T, T, 0, 0});
    L2.push_back({a1, T, t.ae2.w, t.ae2.b, ea, T, B, T, T, 0, 0});
    // encoder hidden states [B][1][cross] -> fp32 (through the fp16 copy the other plans take)
    const size_t ne = (size_t)B * cross;
    half_t* e16 = cx.h(ne);
    float* e32 = cx.f(ne);
    RUN(cx, op_nchw_to_nhwc(a.ehs, a.ehs_dt, e16, 1, 1, (int)ne, cx.s));
    RUN(cx, op_nhwc_to_nchw(e16, e32, DT_F32, 1, 1, (int)ne, 1.f, cx.s));
    P->e.h16 = e16; P->e.f32 = e32; P->e.batch = B; P->e.Lk = 1; P->e.cross = cross;
    // the transformers in forward order
    std::vector<const UTfmW*> tf;
    for (const UBlockW& d : t.down) for (const UTfmW& w : d.attn) tf.push_back(&w);
    for (const UTfmW& w : t.mid.attn) tf.push_back(&w);
    for (const UBlockW& u : t.up) for (const UTfmW& w : u.attn) tf.push_back(&w);
    P->tf.assign(tf.size(), TfmPre());
    std::vector<std::pair<int, float*>> fs;            // frame-index sinusoids shared by the transformers of one width
    for (size_t i = 0; i < tf.size(); ++i) {
        const UTfmW& w = *tf[i];
        const int C = w.C;
        float* fsin = nullptr;
        for (auto& kv : fs) if (kv.first == C) fsin = kv.second;
        if (!fsin) {
            fsin = cx.f((size_t)F * C);
            RUN(cx, op_frameidx_sincos(fsin, F, F, C, cx.s));
            fs.push_back({C, fsin});
        }
        float* f1 = cx.f((size_t)F * 4 * C);
        float* femb = cx.f((size_t)F * C);
        L1.push_back({fsin, C, w.tpe1.w, w.tpe1.b, f1, 4 * C, F, 4 * C, C, 0, 1});
        L2.push_back({f1, 4 * C, w.tpe2.w, w.tpe2.b, femb, C, F, C, 4 * C, 0, 0});
        P->tf[i].femb = femb;
        auto one_key = [&](const AttnW& aw, std::vector<const float*>* dst) {
            float* v = cx.f((size_t)B * aw.inner);
            float* o = cx.f((size_t)B * C);
            L1.push_back({e32, cross, aw.v.w, nullptr, v, aw.inner, B, aw.inner, cross, 0, 0});
            L2.push_back({v, aw.inner, aw.out.w, aw.out.b, o, C, B, C, aw.inner, 0, 0});
            dst->push_back(o);
        };
        for (size_t k = 0; k < w.tb.size(); ++k) {
            one_key(w.tb[k].attn2, &P->tf[i].s_ov);
            one_key(w.ttb[k].attn2, &P->tf[i].t_ov);
        }
    }
    RUN(cx, op_linear_small_group(L1.data(), (int)L1.size(), cx.s));
    RUN(cx, op_linear_small_group(L2.data(), (int)L2.size(), cx.s));
    // emb = time_embedding + add_embedding; every ResNet starts with SiLU(emb): applied on load by the batched projection
    float* emb = cx.f((size_t)B * T);
    RUN(cx, op_add_rowvec(et, DT_F32, ea, T, emb, DT_F32, (size_t)B, T, 1, B, cx.s));
    P->tproj = cx.f((size_t)B * t.temb_total);
    RUN(cx, op_linear_small(emb, T, t.temb_cat.w, t.temb_cat.b, P->tproj, t.temb_total, B, t.temb_total, T, 1, 0, cx.s));
    return 0;
}

// out (row stride ldo) = SpatioTemporalResBlock(x) over B clips of F frames at h x w; x dense [M][Cin]
int run_st_res(Ctx& cx, const UNetST& t, const USTResW& w, const TV& x, const TV& out, long ldo, const UFwd& a, int h, int wd, const Pre& P) {
    const int B = a.B, F = a.F, N = B * F, HW = h * wd, M = N * HW, C = w.sp.Cout, ld = t.temb_total;
    const size_t mk = cx.mark();
    TV xs = stream_alloc(cx, (size_t)M * C, false);                        // x_spatial
    TRY(run_resnet(cx, w.sp, x, xs, N, h, wd, 1, P.tproj + w.toff_s, ld, w.eps, 0, F * HW));
    const bool sd = w.tc1.dup;                                              // split operand: rows [hi | lo], the weights packed twice
    const int K = w.tc1.Cin;                                                // C, or 2 C
    half_t* n1 = cx.h((size_t)M * K);
    TRY(run_groupnorm(cx, w.tn1, xs, n1, B, F * HW, w.eps, true, sd));      // statistics span the clip's frames
    TV h1 = stream_alloc(cx, (size_t)M * C, false);
    IGemmArgs g = {};
    g.A = n1; g.lda = K; g.mode = IG_TEMPORAL; g.Cin = K; g.taps = 3; g.F = F; g.HW = HW; g.t_pad = 0; g.a_split = sd ? 1 : 0;
    g.W = w.tc1.w; g.M = M; g.Nout = C; g.Ktot = 3 * K; g.bias = w.tc1.b;
    g.rowvec = P.tproj + w.toff_t; g.rowvec_ld = ld; g.rows_per_img = F * HW; g.scale = 1.f;
    set_out(g, h1, C, C);
    RUN(cx, op_igemm(g, cx.s));
    TRY(run_groupnorm(cx, w.tn2, h1, n1, B, F * HW, w.eps, true, sd));
    IGemmArgs g2 = g;
    g2.W = w.tc2.w; g2.bias = w.tc2.b; g2.rowvec = nullptr; g2.rowvec_ld = 0; g2.rows_per_img = HW;
    set_res(g2, xs, C);
    set_out(g2, out, ldo, C);
    set_blend(g2, w.mix, xs, C);
    RUN(cx, op_igemm(g2, cx.s));
    cx.release(mk);
    return 0;
}

// TemporalBasicTransformerBlock on frame-major tokens X [(b f) L][dim] (the unsharded core of the adapter's runner, with the UNet's
// inner width = dim, whose feed-forwards take the two-launch GEGLU path); X_ln = norm_in(X)
int run_temporal_tb(Ctx& cx, const TemporalTBW& w, const TV& X, const TV& out, int B, int F, int L, const float* blend_mix,
                    const TV& blend_other, const float* ov, half_t* X_ln) {
    const size_t mk = cx.mark();
    const int M = B * F * L, dim = w.dim, Ci = w.attn1.inner;
    half_t* xn = X_ln;
    TV x0 = stream_alloc(cx, (size_t)M * dim, false);
    TRY(run_ffn(cx, w.ffin1, w.ffin2, xn, dim, x0, M, X, nullptr, TV(), &w.norm1, xn));
    half_t* qkv = cx.h((size_t)M * 3 * Ci);
    TRY(run_linear(cx, w.attn1.qkv, xn, dim, tv16(qkv), 3 * Ci, M, TV(), 0));
    half_t* o = cx.h((size_t)M * Ci);
    TAttnArgs ta = {};
    ta.Q = qkv; ta.ld = 3 * Ci; ta.O = o; ta.ldo = Ci; ta.Bc = B; ta.F = F; ta.HW = L; ta.heads = w.attn1.heads;
    ta.scale = 0.125f;
    RUN(cx, op_temporal_attn(ta, cx.s));
    TV x2 = stream_alloc(cx, (size_t)M * dim, false);
    if (B > 1) {
        // one context per clip: row (b f p) takes the vector of clip (b L + p) % B (the reference's pairing)
        RUN(cx, op_add_rowvec_clip(x0.p, x0.dt, ov, dim, x0.p, x0.dt, B, F, L, dim, cx.s));
        ov = nullptr;
    }
    TRY(run_linear(cx, w.attn1.out, o, Ci, x2, dim, M, x0, dim, ov, ov ? dim : 0, ov ? M : 0, nullptr, TV(), &w.norm3, xn));
    TRY(run_ffn(cx, w.ff1, w.ff2, xn, dim, out, M, x2, blend_mix, blend_other));
    cx.release(mk);
    return 0;
}

// out (row stride ldo) = TransformerSpatioTemporalModel(x); x dense [M][C]
int run_tfm(Ctx& cx, const UTfmW& w, const TV& x, const TV& out, long ldo, const UFwd& a, int h, int wd, Pre& P) {
    const int B = a.B, F = a.F, N = B * F, L = h * wd, M = N * L, C = w.C;
    const TfmPre& tp = P.tf[P.next++];
    const size_t mk = cx.mark();
    half_t* n = cx.h((size_t)M * C);
    TRY(run_groupnorm(cx, w.norm, x, n, N, L, 1e-6f, false));
    TV tok = stream_alloc(cx, (size_t)M * C, false);
    half_t* tok_ln = cx.h((size_t)M * C);
    TRY(run_linear(cx, w.proj_in, n, C, tok, C, M, TV(), 0, nullptr, 0, 0, nullptr, TV(), &w.tb[0].norm1, tok_ln));
    const size_t nk = w.tb.size();
    for (size_t k = 0; k < nk; ++k) {
        TV t2 = stream_alloc(cx, (size_t)M * C, false);
        TRY(run_basic_tb(cx, w.tb[k], tok, t2, N, L, P.e, tp.s_ov[k], nullptr, k == 0 ? tok_ln : nullptr, F * L));
        // + frame-index embedding, and the temporal block's first LayerNorm, in one pass
        TV t3 = stream_alloc(cx, (size_t)M * C, false);
        half_t* t3_ln = cx.h((size_t)M * C);
        RUN(cx, op_layernorm_add(t2.p, t2.dt, C, tp.femb, C, L, F, t3.p, w.ttb[k].norm_in.g, w.ttb[k].norm_in.b, t3_ln, C, M, C, 1e-5f, cx.s));
        // AlphaBlender folded into the temporal block's last GEMM; behind the last layer the blend is proj_out's operand only: fp16
        TV t5 = k + 1 == nk ? tv16(cx.h((size_t)M * C)) : stream_alloc(cx, (size_t)M * C, false);
        TRY(run_temporal_tb(cx, w.ttb[k], t3, t5, B, F, L, w.mix, t2, tp.t_ov[k], t3_ln));
        tok = t5;
    }
    TRY(run_linear(cx, w.proj_out, tok.m16, C, out, ldo, M, x, C));
    cx.release(mk);
    return 0;
}

TV stream_f32(Ctx& cx, size_t rows, int C, bool need16) {
    TV t;
    t.p = cx.f(rows * C); t.dt = DT_F32;
    t.m16 = need16 ? cx.h(rows * C) : nullptr;
    return t;
}

struct Skip { TV x; int C, h, w; };

int unet_run(Ctx& cx, const UNetST& t, const UFwd& a) {
    const ctrl_unet_st_config& c = t.cfg;
    const int nl = c.num_levels, B = a.B, F = a.F, N = B * F, C0 = c.block_out_channels[0];
    cx.stats_off = 0;
    TRY(begin_forward(cx));
    Pre P;
    TRY(precompute(cx, t, a, &P));
    // ---- conv_in: NCHW sample -> the fp32 stream ----
    int h = a.h, w = a.w;
    std::vector<Skip> skips;
    TV cur = stream_f32(cx, (size_t)N * h * w, C0, false);
    RUN(cx, op_conv3x3_direct_f32(a.sample, a.dt, t.conv_in.w, t.conv_in.b, (float*)cur.p, N, c.in_channels, C0, h, w, cx.s));
    skips.push_back({cur, C0, h, w});
    // ---- down blocks ----
    for (int i = 0; i < nl; ++i) {
        const UBlockW& d = t.down[i];
        const int C = d.Cout, nres = (int)d.res.size();
        for (int j = 0; j < nres; ++j) {
            const bool to_conv = j + 1 == nres && d.resample;         // the down-sampler reads the fp16 mirror
            const size_t rows = (size_t)N * h * w;
            TV y = stream_f32(cx, rows, C, to_conv);
            if (d.attn.empty()) {
                TRY(run_st_res(cx, t, d.res[j], cur, y, C, a, h, w, P));
            } else {
                const size_t mk = cx.mark();
                TV r = stream_f32(cx, rows, C, false);
                TRY(run_st_res(cx, t, d.res[j], cur, r, C, a, h, w, P));
                TRY(run_tfm(cx, d.attn[j], r, y, C, a, h, w, P));
                cx.release(mk);
            }
            cur = y;
            skips.push_back({cur, C, h, w});
        }
        if (d.resample) {
            const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
            TV y = stream_f32(cx, (size_t)N * ho * wo, C, t.down[i + 1].res[0].sp.has_shortcut);
            ConvOpts o; o.stride = 2;
            TRY(run_conv(cx, d.conv, cur.m16, y, N, h, w, o));
            cur = y; h = ho; w = wo;
            skips.push_back({cur, C, h, w});
        }
    }
    // ---- mid block; its output is the h half of the first up ResNet's operand ----
    size_t si = skips.size();
    auto alloc_cat = [&](size_t rows, int C1) { return stream_f32(cx, rows, C1 + skips[si - 1].C, true); };
    const int Cm = t.mid.Cout;
    TV cat = alloc_cat((size_t)N * h * w, Cm);
    int C1 = Cm;
    {
        const size_t mk = cx.mark();
        const size_t rows = (size_t)N * h * w;
        TV m0 = stream_f32(cx, rows, Cm, false), m1 = stream_f32(cx, rows, Cm, false);
        TRY(run_st_res(cx, t, t.mid.res[0], cur, m0, Cm, a, h, w, P));
        TRY(run_tfm(cx, t.mid.attn[0], m0, m1, Cm, a, h, w, P));
        TRY(run_st_res(cx, t, t.mid.res[1], m1, cat, Cm + skips[si - 1].C, a, h, w, P));
        cx.release(mk);
    }
    if (a.mid_res)      // :486-489, in place over the mid stream
        RUN(cx, op_unet_skip_join((const float*)cat.p, Cm + skips[si - 1].C, a.mid_res, a.mid_dt, a.mid_5d, B, F, h * w, Cm, (float*)cat.p,
                                  cat.m16, Cm + skips[si - 1].C, 0, cx.s));
    // ---- up blocks ----
    TV fin;
    for (int i = 0; i < nl; ++i) {
        const UBlockW& u = t.up[i];
        const int C = u.Cout, nres = (int)u.res.size();
        for (int j = 0; j < nres; ++j) {
            CTRL_CHECK(si >= 1, "unet_st: skip bookkeeping");
            const Skip& sk = skips[--si];
            CTRL_CHECK(sk.h == h && sk.w == w && C1 + sk.C == u.res[j].sp.Cin, "unet_st: skip shape bookkeeping");
            const int Ct = C1 + sk.C;
            const void* res = (int)si < a.n_down_res ? a.down_res[si] : nullptr;       // zip(): skip i takes residual i
            RUN(cx, op_unet_skip_join((const float*)sk.x.p, sk.C, res, a.down_dt, a.down_5d, B, F, h * w, sk.C, (float*)cat.p, cat.m16, Ct, C1, cx.s));
            const size_t rows = (size_t)N * h * w;
            const bool last = j + 1 == nres;
            // where this layer's output goes: the h half of the next operand, the up-sampler's operand, or the head
            TV dst; long ldd = C;
            if (!last) { dst = alloc_cat(rows, C); ldd = C + skips[si - 1].C; }
            else dst = stream_f32(cx, rows, C, u.resample);
            if (u.attn.empty()) {
                TRY(run_st_res(cx, t, u.res[j], cat, dst, ldd, a, h, w, P));
            } else {
                const size_t mk = cx.mark();
                TV r = stream_f32(cx, rows, C, false);
                TRY(run_st_res(cx, t, u.res[j], cat, r, C, a, h, w, P));
                TRY(run_tfm(cx, u.attn[j], r, dst, ldd, a, h, w, P));
                cx.release(mk);
            }
            if (!last) { cat = dst; C1 = C; }
            else fin = dst;
        }
        if (u.resample) {
            cat = alloc_cat((size_t)N * 4 * h * w, C);
            ConvOpts o; o.up = 2; o.ldy = C + skips[si - 1].C;
            o.phase = u.conv.w_phase != nullptr && !policy_is0(P_CONV_UP_PHASE);
            TRY(run_conv(cx, u.conv, fin.m16, cat, N, h, w, o));
            h *= 2; w *= 2; C1 = C;
        }
    }
    CTRL_CHECK(si == 0 && h == a.h && w == a.w, "unet_st: skip bookkeeping");
    // ---- conv_norm_out + SiLU + conv_out -> NCHW in the sample's dtype ----
    half_t* nf = cx.h((size_t)N * h * w * C0);
    TRY(run_groupnorm(cx, t.norm_out, fin, nf, N, h * w, 1e-5f, true));
    RUN(cx, op_unet_conv_out(nf, t.conv_out.w, t.conv_out.b, a.out, a.dt, N, h, w, C0, c.out_channels, cx.s));
    return 0;
}

int forward(UNetST& t, const UFwd& a, hipStream_t s) {
    const ctrl_unet_st_config& c = t.cfg;
    CTRL_CHECK(a.sample && a.t && a.ehs && a.add_ids && a.out, "unet_st_forward: null argument");
    CTRL_CHECK(a.dt == DT_F32 || a.dt == DT_F16 || a.dt == DT_BF16, "unet_st_forward: the sample must be fp32, fp16 or bf16");
    CTRL_CHECK(a.ehs_dt == DT_F32 || a.ehs_dt == DT_F16 || a.ehs_dt == DT_BF16, "unet_st_forward: encoder_hidden_states must be fp32, fp16 or bf16");
    CTRL_CHECK(a.B >= 1 && a.B <= 64 && a.F >= 1 && a.F <= 32, "unet_st_forward: 1 .. 64 clips of 1 .. 32 frames (the temporal attention's limit)");
    const int m = 1 << (c.num_levels - 1);
    CTRL_CHECK(a.h >= m && a.w >= m && a.h % m == 0 && a.w % m == 0, "unet_st_forward: the latent height and width must be multiples of 2^(levels - 1)");
    CTRL_CHECK((double)a.B * a.F * a.h * a.w * 2.0 * c.block_out_channels[0] < 2147483648.0,
               "unet_st_forward: the clip batch is too large (frames x pixels x concatenated channels must stay below 2^31 elements)");
    CTRL_CHECK(a.t_count == 1 || a.t_count == a.B, "unet_st_forward: need 1 or B timesteps");
    CTRL_CHECK(a.n_ids * c.addition_time_embed_dim == c.projection_class_embeddings_input_dim,
               "unet_st_forward: added_time_ids must hold projection_class_embeddings_input_dim / addition_time_embed_dim values per clip");
    CTRL_CHECK(a.n_down_res >= 0 && (a.n_down_res == 0 || a.down_res), "unet_st_forward: bad residual list");
    for (int i = 0; i < a.n_down_res; ++i) CTRL_CHECK(a.down_res[i] != nullptr, "unet_st_forward: null residual");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    t.ar.off = 0; t.ar.peak = 0;
    Ctx dry{&t.ar, s, true};
    TRY(unet_run(dry, t, a));
    TRY(t.reserve(workspace_bytes(dry), capturing, "unet_st", "size"));
    t.ar.off = 0;
    Ctx cx{&t.ar, s, false};
    cx.capturing = capturing;
    cx.stats_total = dry.stats_total;
    TRY(unet_run(cx, t, a));
    return t.leave(s, capturing);
}

}  // namespace

extern "C" {

int ctrl_unet_st_param_count(const ctrl_unet_st_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_unet_st_param_spec(const ctrl_unet_st_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "unet_st_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "unet_st_param_spec", name, name_len, shape, ndim);
}

int ctrl_unet_st_create(const ctrl_unet_st_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet_st** out) {
    return plan_create<UNetST>("unet_st_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_unet,
                               [](UNetST&, hipStream_t) { return 0; });
}

void ctrl_unet_st_destroy(ctrl_unet_st* h) { plan_destroy<UNetST>(h); }

int ctrl_unet_st_selection(ctrl_unet_st* h, char* buf, int len) {
    CTRL_CHECK(h && buf && len > 0, "unet_st_selection: null argument");
    const UNetST* t = (const UNetST*)h;
    bool phase = false;
    for (const UBlockW& u : t->up) phase = phase || (u.resample && u.conv.w_phase);
    snprintf(buf, (size_t)len, "streams=fp32 resnet_split_operands=%d upsampler_phase_pack=%d time_projection_columns=%d selection=default",
             t->split ? 1 : 0, phase ? 1 : 0, t->temb_total);
    return 0;
}

int ctrl_unet_st_forward(ctrl_unet_st* h, const void* sample, int sample_dtype, int B, int F, int lat_h, int lat_w, const float* timesteps,
                         int t_count, const void* encoder_hidden_states, int ehs_dtype, const float* added_time_ids, int n_time_ids,
                         const void* const* down_residuals, int n_down_residuals, int down_dtype, int down_5d, const void* mid_residual,
                         int mid_dtype, int mid_5d, void* out, void* stream) {
    CTRL_CHECK(h != nullptr, "unet_st_forward: null plan");
    UNetST* t = (UNetST*)h;
    DeviceGuard dg(t->device);
    const UFwd a = {sample, sample_dtype, B, F, lat_h, lat_w, timesteps, t_count, encoder_hidden_states, ehs_dtype, added_time_ids, n_time_ids,
                    down_residuals, n_down_residuals, down_dtype, down_5d, mid_residual, mid_dtype, mid_5d, out};
    return forward(*t, a, S(stream));
}

int ctrl_op_unet_skip_join(const float* skip, int64_t ld_skip, const void* res, int res_dtype, int res_5d, int B, int F, int HW, int C2,
                           float* out32, void* out16, int64_t ld_out, int col, void* stream) {
    return op_unet_skip_join(skip, (long)ld_skip, res, res_dtype, res_5d, B, F, HW, C2, out32, (half_t*)out16, (long)ld_out, col, S(stream));
}

int ctrl_op_unet_skip_join_split(const float* skip, int64_t ld_skip, const void* res, int res_dtype, int res_5d, int B, int F, int HW, int C2,
                                 float* out32, void* out16, int64_t ld_out, int col, int lo_off, void* stream) {
    return op_unet_skip_join(skip, (long)ld_skip, res, res_dtype, res_5d, B, F, HW, C2, out32, (half_t*)out16, (long)ld_out, col, S(stream),
                             lo_off);
}

}  // extern "C"
