// SDXL backbone UNet plan: diffusers' UNet2DConditionModel in the configuration family SDXL-base uses (addition_embed_type "text_time",
// use_linear_projection, a transformer depth per level; called at sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1356-1366).
// Order of operations, after diffusers' forward:
//   time_proj -> time_embedding | add_time_proj(time_ids.flatten()) reshaped per sample, concat([text_embeds, time_embeds]) ->
//   add_embedding, summed | every ResNet's time_emb_proj(SiLU(emb)) as ONE small-M linear | the K / V^T projections of
//   encoder_hidden_states for every cross-attention of the forward (project_text_kv, the plan's text cache) | conv_in | down blocks
//   collecting the skips | mid block (ResNet, transformer, ResNet) | the residuals | up blocks over the REVERSED per-level lists |
//   conv_norm_out + SiLU + conv_out, NCHW in the sample's dtype.
// Transformer2DModel (use_linear_projection): GroupNorm (eps 1e-6), proj_in, depth x BasicTransformerBlock, proj_out + input.
// Activations are channels-last [(b) h w][C]; residual streams fp32, fp16 mirrors where a GEMM reads them.  The up path never
// concatenates (as plan_unet_st.cpp): the operand [rows][C1 + C2] of an up ResNet is allocated first, the producer of its h half writes
// columns [0, C1) through the output row stride, op_unet_skip_join (F = 1, 4-D residuals) writes the skip (+ the adapter's residual)
// into columns [C1, C1 + C2).  Upsample2D is the implicit GEMM's 9-tap gather (up = 2); the phase form is not used here.
// Main-path operands are split: the convolutions that carry the WHOLE stream rather than a residual branch -- the 1x1 shortcut of
// every ResNet that changes width (all of the up path's: they read the concatenation), the down-samplers and the up-samplers -- take
// their A operand as [hi | lo] fp16 halves of the fp32 stream (exact to ~2^-22 instead of 2^-11).  An fp16 operand costs every
// output a relative error of ~2.8e-4 rms, whatever K is; on a branch that is diluted by the skip path, on these convolutions it is
// the stream itself, fifteen times over between conv_in and conv_out at SDXL's config.  The 1x1 shortcuts are a ninth of a 3x3's work, the samplers are
// three launches at SDXL's config.  So every fp16 mirror of a stream in this plan is a [hi | lo] row pair, 2 C wide (stream_f32).
// One stream, no lanes, no grouped launches: capturable as a linear graph.
#include "plan_common.h"
#include <cstdio>

namespace {

struct U2ResW { ResnetW r; int toff = 0; };      // toff: columns of time_emb_proj inside the batched projection

struct U2TfmW {                  // Transformer2DModel, linear projections
    Norm norm;
    Lin proj_in, proj_out;
    std::vector<BasicTBW> tb;
    int C = 0;
};

struct U2BlockW {
    std::vector<U2ResW> res;
    std::vector<U2TfmW> attn;    // empty: a block without attention
    bool resample = false;
    ConvW conv;                  // downsamplers.0.conv | upsamplers.0.conv
    int Cout = 0;
};

struct UNet2D : StandalonePlan {
    ctrl_unet2d_config cfg{};
    ConvD conv_in, conv_out;
    Lin te1, te2, ae1, ae2, temb_cat;
    std::vector<U2BlockW> down, up;
    U2BlockW mid;
    Norm norm_out;
    int temb_total = 0, n_cross = 0;
    KvCache kvc;                 // text K/V cache (ctrl_unet2d_set_text_cache)
    // split [hi | lo] operands for the 3x3 convolutions of every ResNet (CTRL_UNET_SPLIT=1, read at plan creation, as in plan_unet_st.cpp):
    // their operand is a GroupNorm output, exact to ~2^-22 instead of 2^-11 at twice the matrix work of those launches.  Off by default
    bool split = false;
    std::vector<std::string> temb_names;
    std::vector<int> temb_ns;
};

int validate(const ctrl_unet2d_config& c) {
    CTRL_CHECK(c.num_levels >= 1 && c.num_levels <= 4, "unet2d: 1 .. 4 levels");
    CTRL_CHECK(c.in_channels == 4 || c.in_channels == 8, "unet2d: in_channels must be 4 or 8 (the stem kernel's instantiations)");
    CTRL_CHECK(c.out_channels >= 1 && c.out_channels <= 4, "unet2d: out_channels must be 1 .. 4");
    CTRL_CHECK(c.layers_per_block >= 1 && c.layers_per_block <= 4, "unet2d: layers_per_block out of range");
    for (int i = 0; i < c.num_levels; ++i) {
        const int C = c.block_out_channels[i];
        CTRL_CHECK(C >= 64 && C % 64 == 0 && C <= 2048, "unet2d: block_out_channels must be multiples of 64 up to 2048");
        const bool attends = c.level_has_attn[i] || i + 1 == c.num_levels;
        CTRL_CHECK(!attends || (c.num_attention_heads[i] >= 1 && C == 64 * c.num_attention_heads[i]),
                   "unet2d: attention_head_dim (out_channels / heads) must be 64 at every attention level and in the mid block");
        CTRL_CHECK(!attends || (c.transformer_layers_per_block[i] >= 1 && c.transformer_layers_per_block[i] <= 16),
                   "unet2d: transformer_layers_per_block must be 1 .. 16 at every attention level and in the mid block");
    }
    CTRL_CHECK(c.cross_attention_dim >= 8 && c.cross_attention_dim % 8 == 0, "unet2d: cross_attention_dim must be a multiple of 8");
    CTRL_CHECK(c.addition_time_embed_dim >= 8 && c.addition_time_embed_dim % 8 == 0 && c.projection_class_embeddings_input_dim % 8 == 0 &&
                   c.projection_class_embeddings_input_dim > c.addition_time_embed_dim,
               "unet2d: addition_time_embed_dim and projection_class_embeddings_input_dim must be multiples of 8, the second the larger");
    CTRL_CHECK(c.norm_eps > 0.f && c.norm_eps < 1.f, "unet2d: norm_eps out of range");
    return 0;
}

int build_res(ParamSink& ps, UNet2D& t, const std::string& pre, int Cin, int Cout, U2ResW* w) {
    TRY(build_resnet(ps, pre, Cin, Cout, false, &w->r, t.split, /*shortcut: split, it carries the stream*/ 1));
    w->toff = t.temb_total; t.temb_total += Cout;
    t.temb_names.push_back(pre + ".time_emb_proj"); t.temb_ns.push_back(Cout);
    return 0;
}

int build_tfm(ParamSink& ps, UNet2D& t, const std::string& pre, int C, int heads, int depth, U2TfmW* w) {
    w->C = C;
    TRY(ps.norm(pre + ".norm", C, &w->norm));
    TRY(ps.linear(pre + ".proj_in", C, C, true, false, &w->proj_in));
    w->tb.resize(depth);
    for (int k = 0; k < depth; ++k)
        TRY(build_basic_tb(ps, pre + ".transformer_blocks." + std::to_string(k), C, heads, 64, t.cfg.cross_attention_dim, &w->tb[k]));
    TRY(ps.linear(pre + ".proj_out", C, C, true, false, &w->proj_out));
    t.n_cross += depth;
    return 0;
}

int build_unet(ParamSink& ps, UNet2D& t) {
    const ctrl_unet2d_config& c = t.cfg;
    const int nl = c.num_levels, C0 = c.block_out_channels[0], T = 4 * C0;
    t.temb_total = 0; t.n_cross = 0; t.temb_names.clear(); t.temb_ns.clear();
    t.split = policy_is1(P_UNET_SPLIT);
    TRY(ps.conv_direct("conv_in", C0, c.in_channels, &t.conv_in));
    TRY(ps.linear("time_embedding.linear_1", T, C0, true, false, &t.te1));
    TRY(ps.linear("time_embedding.linear_2", T, T, true, false, &t.te2));
    TRY(ps.linear("add_embedding.linear_1", T, c.projection_class_embeddings_input_dim, true, false, &t.ae1));
    TRY(ps.linear("add_embedding.linear_2", T, T, true, false, &t.ae2));
    // down blocks; the skip channels in the order diffusers collects them
    std::vector<int> skip_c = {C0};
    t.down.resize(nl);
    int cin = C0;
    for (int i = 0; i < nl; ++i) {
        U2BlockW& d = t.down[i];
        const std::string pre = "down_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[i] != 0;
        d.Cout = c.block_out_channels[i];
        d.res.resize(c.layers_per_block);
        if (attn) d.attn.resize(c.layers_per_block);
        for (int j = 0; j < c.layers_per_block; ++j) {
            TRY(build_res(ps, t, pre + ".resnets." + std::to_string(j), j == 0 ? cin : d.Cout, d.Cout, &d.res[j]));
            if (attn) TRY(build_tfm(ps, t, pre + ".attentions." + std::to_string(j), d.Cout, c.num_attention_heads[i],
                                    c.transformer_layers_per_block[i], &d.attn[j]));
            skip_c.push_back(d.Cout);
        }
        d.resample = i + 1 < nl;
        if (d.resample) {
            TRY(ps.conv(pre + ".downsamplers.0.conv", d.Cout, d.Cout, 3, false, &d.conv, /*split*/ true));
            skip_c.push_back(d.Cout);
        }
        cin = d.Cout;
    }
    // UNetMidBlock2DCrossAttn: ResNet, transformer (the last level's heads and depth), ResNet
    {
        const int Cm = c.block_out_channels[nl - 1];
        t.mid.Cout = Cm;
        t.mid.res.resize(2);
        t.mid.attn.resize(1);
        TRY(build_res(ps, t, "mid_block.resnets.0", Cm, Cm, &t.mid.res[0]));
        TRY(build_tfm(ps, t, "mid_block.attentions.0", Cm, c.num_attention_heads[nl - 1], c.transformer_layers_per_block[nl - 1], &t.mid.attn[0]));
        TRY(build_res(ps, t, "mid_block.resnets.1", Cm, Cm, &t.mid.res[1]));
    }
    // up blocks: layers_per_block + 1 ResNets over [h | skip]; heads and depth from the reversed per-level lists
    t.up.resize(nl);
    int prev = c.block_out_channels[nl - 1];
    size_t si = skip_c.size();
    for (int i = 0; i < nl; ++i) {
        U2BlockW& u = t.up[i];
        const int li = nl - 1 - i;
        const std::string pre = "up_blocks." + std::to_string(i);
        const bool attn = c.level_has_attn[li] != 0;
        u.Cout = c.block_out_channels[li];
        u.res.resize(c.layers_per_block + 1);
        if (attn) u.attn.resize(c.layers_per_block + 1);
        for (int j = 0; j <= c.layers_per_block; ++j) {
            const int cskip = skip_c[--si];
            TRY(build_res(ps, t, pre + ".resnets." + std::to_string(j), (j == 0 ? prev : u.Cout) + cskip, u.Cout, &u.res[j]));
            if (attn) TRY(build_tfm(ps, t, pre + ".attentions." + std::to_string(j), u.Cout, c.num_attention_heads[li],
                                    c.transformer_layers_per_block[li], &u.attn[j]));
        }
        u.resample = i + 1 < nl;
        if (u.resample) TRY(ps.conv(pre + ".upsamplers.0.conv", u.Cout, u.Cout, 3, false, &u.conv, /*split*/ true));     // (no phase pack: the 9-tap gather)
        prev = u.Cout;
    }
    CTRL_CHECK(si == 0, "unet2d: skip bookkeeping");
    TRY(ps.norm("conv_norm_out", C0, &t.norm_out));
    TRY(ps.conv_direct("conv_out", c.out_channels, C0, &t.conv_out));
    TRY(ps.linear_cat(t.temb_names, t.temb_ns, T, true, &t.temb_cat));
    return 0;
}

int collect(const ctrl_unet2d_config& c, SpecCollector& sc) {
    TRY(validate(c));
    UNet2D t;
    t.cfg = c;
    return build_unet(sc, t);
}

struct UFwd {
    const void* sample; int dt; int B, h, w;
    const float* t; int t_count;
    const void* ehs; int ehs_dt, Lk;
    const void* text; int text_dt, text_dim;
    const float* ids; int n_ids;
    const void* const* down_res; int n_down_res, down_dt;
    const void* mid_res; int mid_dt;
    void* out;
};

struct Pre {
    float* tproj = nullptr;                 // [B][temb_total]
    std::vector<PreKV> kv;                  // one per cross-attention, in forward order
    size_t next = 0;
    EhsCtx e;
};

// everything that depends on (timestep, text_embeds, time_ids, encoder_hidden_states) only
int precompute(Ctx& cx, const UNet2D& t, const UFwd& a, Pre* P) {
    const ctrl_unet2d_config& c = t.cfg;
    const int B = a.B, C0 = c.block_out_channels[0], T = 4 * C0, cross = c.cross_attention_dim;
    const int AD = c.addition_time_embed_dim, PD = c.projection_class_embeddings_input_dim;
    std::vector<SmallLin> L1, L2;
    float* tsin = cx.f((size_t)B * C0);
    RUN(cx, op_timestep_sincos(a.t, a.t_count, tsin, B, C0, cx.s));
    float* arow = cx.f((size_t)B * PD);                 // [text_embeds | sinusoids of the time ids]: text first
    RUN(cx, op_unet_text_time(a.text, a.text_dt, a.text_dim, a.ids, a.n_ids, AD, arow, PD, B, cx.s));
    float* t1 = cx.f((size_t)B * T); float* a1 = cx.f((size_t)B * T);
    float* et = cx.f((size_t)B * T); float* ea = cx.f((size_t)B * T);
    L1.push_back({tsin, C0, t.te1.w, t.te1.b, t1, T, B, T, C0, 0, 1});
    L1.push_back({arow, PD, t.ae1.w, t.ae1.b, a1, T, B, T, PD, 0, 1});
    L2.push_back({t1, T, t.te2.w, t.te2.b, et, T, B, T, T, 0, 0});
    L2.push_back({a1, T, t.ae2.w, t.ae2.b, ea, T, B, T, T, 0, 0});
    RUN(cx, op_linear_small_group(L1.data(), (int)L1.size(), cx.s));
    RUN(cx, op_linear_small_group(L2.data(), (int)L2.size(), cx.s));
    // emb = time_embedding + add_embedding; every ResNet starts with SiLU(emb): applied on load by the batched projection
    float* emb = cx.f((size_t)B * T);
    RUN(cx, op_add_rowvec(et, DT_F32, ea, T, emb, DT_F32, (size_t)B, T, 1, B, cx.s));
    P->tproj = cx.f((size_t)B * t.temb_total);
    RUN(cx, op_linear_small(emb, T, t.temb_cat.w, t.temb_cat.b, P->tproj, t.temb_total, B, t.temb_total, T, 1, 0, cx.s));
    // encoder hidden states [B][Lk][cross] -> fp16 rows (+ fp32 for the one-key form)
    const size_t ne = (size_t)B * a.Lk * cross;
    half_t* e16 = cx.h(ne);
    RUN(cx, op_nchw_to_nhwc(a.ehs, a.ehs_dt, e16, 1, 1, (int)ne, cx.s));
    P->e.h16 = e16; P->e.batch = B; P->e.Lk = a.Lk; P->e.cross = cross;
    if (a.Lk == 1) {
        float* e32 = cx.f(ne);
        RUN(cx, op_nhwc_to_nchw(e16, e32, DT_F32, 1, 1, (int)ne, 1.f, cx.s));
        P->e.f32 = e32;
        return 0;
    }
    // K / V^T of the text states for every cross-attention of the forward, in forward order
    std::vector<const BasicTBW*> tbs;
    for (const U2BlockW& d : t.down) for (const U2TfmW& w : d.attn) for (const BasicTBW& b : w.tb) tbs.push_back(&b);
    for (const U2TfmW& w : t.mid.attn) for (const BasicTBW& b : w.tb) tbs.push_back(&b);
    for (const U2BlockW& u : t.up) for (const U2TfmW& w : u.attn) for (const BasicTBW& b : w.tb) tbs.push_back(&b);
    P->kv.assign(tbs.size(), PreKV());
    for (size_t i = 0; i < tbs.size(); ++i) TRY(project_text_kv(cx, tbs[i]->attn2, P->e, &P->kv[i]));
    return 0;
}

int run_res(Ctx& cx, const UNet2D& t, const U2ResW& w, const TV& x, const TV& out, long ldo, int B, int h, int wd, const Pre& P) {
    return run_resnet(cx, w.r, x, out, B, h, wd, 1, P.tproj + w.toff, t.temb_total, t.cfg.norm_eps, ldo);
}

// out (row stride ldo) = Transformer2DModel(x); x dense [M][C]
int run_tfm(Ctx& cx, const U2TfmW& w, const TV& x, const TV& out, long ldo, int B, int h, int wd, Pre& P) {
    const int L = h * wd, M = B * L, C = w.C;
    const size_t mk = cx.mark();
    half_t* n = cx.h((size_t)M * C);
    TRY(run_groupnorm(cx, w.norm, x, n, B, L, 1e-6f, false));
    TV tok = stream_alloc(cx, (size_t)M * C, false);
    half_t* tok_ln = cx.h((size_t)M * C);
    TRY(run_linear(cx, w.proj_in, n, C, tok, C, M, TV(), 0, nullptr, 0, 0, nullptr, TV(), &w.tb[0].norm1, tok_ln));
    const size_t nk = w.tb.size();
    for (size_t k = 0; k < nk; ++k) {
        // behind the last layer the tokens are proj_out's operand only: fp16
        TV t2 = k + 1 == nk ? tv16(cx.h((size_t)M * C)) : stream_alloc(cx, (size_t)M * C, false);
        const PreKV* kv = P.kv.empty() ? nullptr : &P.kv[P.next];
        ++P.next;
        TRY(run_basic_tb(cx, w.tb[k], tok, t2, B, L, P.e, nullptr, kv, k == 0 ? tok_ln : nullptr));
        tok = t2;
    }
    TRY(run_linear(cx, w.proj_out, tok.m16, C, out, ldo, M, x, C));
    cx.release(mk);
    return 0;
}

// fp32 stream [rows][C]; its fp16 mirror, where a main-path convolution reads it, is a split [hi | lo] row pair, 2 C wide
TV stream_f32(Ctx& cx, size_t rows, int C, bool need16) {
    TV t;
    t.p = cx.f(rows * C); t.dt = DT_F32;
    if (need16) { t.m16 = cx.h(rows * C * 2); t.lo_off = C; }
    return t;
}

struct Skip { TV x; int C, h, w; };

int unet_run(Ctx& cx, UNet2D& t, const UFwd& a) {
    const ctrl_unet2d_config& c = t.cfg;
    const int nl = c.num_levels, B = a.B, C0 = c.block_out_channels[0];
    cx.stats_off = 0;
    t.kvc.next = 0;
    TRY(begin_forward(cx));
    Pre P;
    TRY(precompute(cx, t, a, &P));
    // ---- conv_in: NCHW sample -> the fp32 stream ----
    int h = a.h, w = a.w;
    std::vector<Skip> skips;
    TV cur = stream_f32(cx, (size_t)B * h * w, C0, false);          // (the first ResNet is C0 -> C0: no shortcut conv reads a mirror)
    RUN(cx, op_conv3x3_direct_f32(a.sample, a.dt, t.conv_in.w, t.conv_in.b, (float*)cur.p, B, c.in_channels, C0, h, w, cx.s));
    skips.push_back({cur, C0, h, w});
    // ---- down blocks ----
    for (int i = 0; i < nl; ++i) {
        const U2BlockW& d = t.down[i];
        const int C = d.Cout, nres = (int)d.res.size();
        for (int j = 0; j < nres; ++j) {
            const bool to_conv = j + 1 == nres && d.resample;         // the down-sampler reads the fp16 mirror
            const size_t rows = (size_t)B * h * w;
            TV y = stream_f32(cx, rows, C, to_conv);
            if (d.attn.empty()) {
                TRY(run_res(cx, t, d.res[j], cur, y, C, B, h, w, P));
            } else {
                const size_t mk = cx.mark();
                TV r = stream_f32(cx, rows, C, false);
                TRY(run_res(cx, t, d.res[j], cur, r, C, B, h, w, P));
                TRY(run_tfm(cx, d.attn[j], r, y, C, B, h, w, P));
                cx.release(mk);
            }
            cur = y;
            skips.push_back({cur, C, h, w});
        }
        if (d.resample) {
            const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
            TV y = stream_f32(cx, (size_t)B * ho * wo, C, t.down[i + 1].res[0].r.has_shortcut);
            ConvOpts o; o.stride = 2;
            TRY(run_conv(cx, d.conv, cur.m16, y, B, h, w, o));
            cur = y; h = ho; w = wo;
            skips.push_back({cur, C, h, w});
        }
    }
    // ---- mid block; its output is the h half of the first up ResNet's operand ----
    size_t si = skips.size();
    auto alloc_cat = [&](size_t rows, int C1) { return stream_f32(cx, rows, C1 + skips[si - 1].C, true); };
    const int Cm = t.mid.Cout;
    TV cat = alloc_cat((size_t)B * h * w, Cm);
    int C1 = Cm;
    {
        const size_t mk = cx.mark();
        const size_t rows = (size_t)B * h * w;
        TV m0 = stream_f32(cx, rows, Cm, false), m1 = stream_f32(cx, rows, Cm, false);
        TRY(run_res(cx, t, t.mid.res[0], cur, m0, Cm, B, h, w, P));
        TRY(run_tfm(cx, t.mid.attn[0], m0, m1, Cm, B, h, w, P));
        TRY(run_res(cx, t, t.mid.res[1], m1, cat, Cm + skips[si - 1].C, B, h, w, P));
        cx.release(mk);
    }
    if (a.mid_res)      // in place over the mid stream
        RUN(cx, op_unet_skip_join((const float*)cat.p, Cm + skips[si - 1].C, a.mid_res, a.mid_dt, 0, B, 1, h * w, Cm, (float*)cat.p, cat.m16,
                                  Cm + skips[si - 1].C, 0, cx.s, cat.lo_off));
    // ---- up blocks ----
    TV fin;
    for (int i = 0; i < nl; ++i) {
        const U2BlockW& u = t.up[i];
        const int C = u.Cout, nres = (int)u.res.size();
        for (int j = 0; j < nres; ++j) {
            CTRL_CHECK(si >= 1, "unet2d: skip bookkeeping");
            const Skip& sk = skips[--si];
            CTRL_CHECK(sk.h == h && sk.w == w && C1 + sk.C == u.res[j].r.Cin, "unet2d: skip shape bookkeeping");
            const int Ct = C1 + sk.C;
            const void* res = (int)si < a.n_down_res ? a.down_res[si] : nullptr;       // zip(): skip i takes residual i
            RUN(cx, op_unet_skip_join((const float*)sk.x.p, sk.C, res, a.down_dt, 0, B, 1, h * w, sk.C, (float*)cat.p, cat.m16, Ct, C1, cx.s, cat.lo_off));
            const size_t rows = (size_t)B * h * w;
            const bool last = j + 1 == nres;
            // where this layer's output goes: the h half of the next operand, the up-sampler's operand, or the head
            TV dst; long ldd = C;
            if (!last) { dst = alloc_cat(rows, C); ldd = C + skips[si - 1].C; }
            else dst = stream_f32(cx, rows, C, u.resample);
            if (u.attn.empty()) {
                TRY(run_res(cx, t, u.res[j], cat, dst, ldd, B, h, w, P));
            } else {
                const size_t mk = cx.mark();
                TV r = stream_f32(cx, rows, C, false);
                TRY(run_res(cx, t, u.res[j], cat, r, C, B, h, w, P));
                TRY(run_tfm(cx, u.attn[j], r, dst, ldd, B, h, w, P));
                cx.release(mk);
            }
            if (!last) { cat = dst; C1 = C; }
            else fin = dst;
        }
        if (u.resample) {
            cat = alloc_cat((size_t)B * 4 * h * w, C);
            ConvOpts o; o.up = 2; o.ldy = C + skips[si - 1].C;
            TRY(run_conv(cx, u.conv, fin.m16, cat, B, h, w, o));
            h *= 2; w *= 2; C1 = C;
        }
    }
    CTRL_CHECK(si == 0 && h == a.h && w == a.w, "unet2d: skip bookkeeping");
    CTRL_CHECK(a.Lk == 1 || P.next == P.kv.size(), "unet2d: cross-attention bookkeeping");
    // ---- conv_norm_out + SiLU + conv_out -> NCHW in the sample's dtype ----
    half_t* nf = cx.h((size_t)B * h * w * C0);
    TRY(run_groupnorm(cx, t.norm_out, fin, nf, B, h * w, c.norm_eps, true));
    RUN(cx, op_unet_conv_out(nf, t.conv_out.w, t.conv_out.b, a.out, a.dt, B, h, w, C0, c.out_channels, cx.s));
    return 0;
}

int forward(UNet2D& t, const UFwd& a, hipStream_t s) {
    const ctrl_unet2d_config& c = t.cfg;
    CTRL_CHECK(a.sample && a.t && a.ehs && a.text && a.ids && a.out, "unet2d_forward: null argument");
    CTRL_CHECK(a.dt == DT_F32 || a.dt == DT_F16 || a.dt == DT_BF16, "unet2d_forward: the sample must be fp32, fp16 or bf16");
    CTRL_CHECK(a.ehs_dt == DT_F32 || a.ehs_dt == DT_F16 || a.ehs_dt == DT_BF16, "unet2d_forward: encoder_hidden_states must be fp32, fp16 or bf16");
    CTRL_CHECK(a.text_dt == DT_F32 || a.text_dt == DT_F16 || a.text_dt == DT_BF16, "unet2d_forward: text_embeds must be fp32, fp16 or bf16");
    CTRL_CHECK(a.B >= 1 && a.B <= 1024 && a.Lk >= 1 && a.Lk <= 65536, "unet2d_forward: 1 .. 1024 samples, 1 .. 65536 keys");
    const int m = 1 << (c.num_levels - 1);
    CTRL_CHECK(a.h >= m && a.w >= m && a.h % m == 0 && a.w % m == 0, "unet2d_forward: the latent height and width must be multiples of 2^(levels - 1)");
    CTRL_CHECK((double)a.B * a.h * a.w * 2.0 * c.block_out_channels[0] < 2147483648.0,
               "unet2d_forward: the batch is too large (pixels x concatenated channels must stay below 2^31 elements)");
    CTRL_CHECK((double)a.B * a.Lk * c.cross_attention_dim < 2147483648.0, "unet2d_forward: encoder_hidden_states too large");
    CTRL_CHECK(a.t_count == 1 || a.t_count == a.B, "unet2d_forward: need 1 or B timesteps");
    CTRL_CHECK(a.text_dim >= 1 && a.n_ids >= 1 &&
                   (long)a.text_dim + (long)a.n_ids * c.addition_time_embed_dim == c.projection_class_embeddings_input_dim,
               "unet2d_forward: text_embeds width + n_time_ids * addition_time_embed_dim must equal projection_class_embeddings_input_dim");
    CTRL_CHECK(a.n_down_res >= 0 && (a.n_down_res == 0 || a.down_res), "unet2d_forward: bad residual list");
    for (int i = 0; i < a.n_down_res; ++i) CTRL_CHECK(a.down_res[i] != nullptr, "unet2d_forward: null residual");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    CTRL_CHECK(!(capturing && t.kvc.mode == KvCache::KEEP && t.kvc.slots.empty()),
               "text K/V cache: the first KEEP forward allocates its buffers and cannot run under stream capture -- run it eagerly once, then capture");
    if (t.kvc.mode == KvCache::REUSE)
        CTRL_CHECK(t.kvc.key_batch == a.B && t.kvc.key_Lk == a.Lk, "unet2d_forward: text K/V cache was kept for another batch / prompt length");
    t.ar.off = 0; t.ar.peak = 0;
    Ctx dry{&t.ar, s, true};
    dry.kvc = &t.kvc;
    TRY(unet_run(dry, t, a));
    TRY(t.reserve(workspace_bytes(dry), capturing, "unet2d", "size"));
    t.ar.off = 0;
    Ctx cx{&t.ar, s, false};
    cx.kvc = &t.kvc;
    cx.capturing = capturing;
    cx.stats_total = dry.stats_total;
    TRY(unet_run(cx, t, a));
    if (t.kvc.mode == KvCache::KEEP) { t.kvc.key_batch = a.B; t.kvc.key_Lk = a.Lk; }
    return t.leave(s, capturing);
}

}  // namespace

extern "C" {

int ctrl_unet2d_param_count(const ctrl_unet2d_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_unet2d_param_spec(const ctrl_unet2d_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "unet2d_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "unet2d_param_spec", name, name_len, shape, ndim);
}

int ctrl_unet2d_create(const ctrl_unet2d_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet2d** out) {
    return plan_create<UNet2D>("unet2d_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_unet,
                               [](UNet2D&, hipStream_t) { return 0; });
}

void ctrl_unet2d_destroy(ctrl_unet2d* h) { plan_destroy<UNet2D>(h); }

int ctrl_unet2d_selection(ctrl_unet2d* h, char* buf, int len) {
    CTRL_CHECK(h && buf && len > 0, "unet2d_selection: null argument");
    const UNet2D* t = (const UNet2D*)h;
    snprintf(buf, (size_t)len, "streams=fp32 main_path_split_operands=1 resnet_split_operands=%d upsampler=gather9 cross_attentions=%d time_projection_columns=%d selection=default",
             t->split ? 1 : 0, t->n_cross, t->temb_total);
    return 0;
}

int ctrl_unet2d_set_text_cache(ctrl_unet2d* h, int mode) {
    CTRL_CHECK(h && mode >= 0 && mode <= 2, "unet2d_set_text_cache: mode must be 0 (off), 1 (keep) or 2 (reuse)");
    ((UNet2D*)h)->kvc.mode = mode;
    return 0;
}

int64_t ctrl_unet2d_workspace_bytes(ctrl_unet2d* h) { return h ? (int64_t)((UNet2D*)h)->ar.cap : -1; }

int ctrl_unet2d_forward(ctrl_unet2d* h, const void* sample, int sample_dtype, int B, int lat_h, int lat_w, const float* timesteps,
                        int t_count, const void* encoder_hidden_states, int ehs_dtype, int Lk, const void* text_embeds, int text_dtype,
                        int text_dim, const float* time_ids, int n_time_ids, const void* const* down_residuals, int n_down_residuals,
                        int down_dtype, const void* mid_residual, int mid_dtype, void* out, void* stream) {
    CTRL_CHECK(h != nullptr, "unet2d_forward: null plan");
    UNet2D* t = (UNet2D*)h;
    DeviceGuard dg(t->device);
    const UFwd a = {sample, sample_dtype, B, lat_h, lat_w, timesteps, t_count, encoder_hidden_states, ehs_dtype, Lk, text_embeds, text_dtype,
                    text_dim, time_ids, n_time_ids, down_residuals, n_down_residuals, down_dtype, mid_residual, mid_dtype, out};
    return forward(*t, a, S(stream));
}

int ctrl_op_unet_text_time(const void* text_embeds, int text_dtype, int text_dim, const float* time_ids, int n_ids, int dim, float* out,
                           int64_t ld_out, int B, void* stream) {
    return op_unet_text_time(text_embeds, text_dtype, text_dim, time_ids, n_ids, dim, out, (long)ld_out, B, S(stream));
}

}  // extern "C"
