// Temporal KL-VAE decoder plan (diffusers v0.27 AutoencoderKLTemporalDecoder.decode = TemporalDecoder: SVD's decode_latents,
// svd/pipelines/svd_controlnet_adapter_pipeline.py:265-292).  The image decoder's dataflow (plan_vae_decoder.cpp) with every ResNet a
// SpatioTemporalResBlock and time_conv_out behind conv_out:
//   head kernel (latents * scale -> conv_in; its post_quant_conv operands are an identity and a zero bias) | mid block: ST-ResNet,
//   then (layers_per_block >= 2) attention per frame, ST-ResNet | per level: layers_per_block + 1 ST-ResNets + Upsample2D on all but the last level | per frame the
//   GroupNorm statistics + the tail kernel (conv_norm_out + SiLU + conv_out, fp32 NCHW into scratch) | time_conv_out + the output
//   epilogue over the clip (vae.hip: vae_time_conv_kernel).
// ST-ResNet = spatial ResnetBlock2D (run_resnet, per frame statistics) -> TemporalResnetBlock on its output x_s (GroupNorm(eps 1e-5)
// whose statistics span the clip's (C / 32, F, H, W), SiLU, Conv3d (3,1,1), the same again, + x_s) -> (1 - a) x_s + a x_t with
// a = sigmoid(mix_factor): the last temporal conv's epilogue carries the fp32 residual x_s and the blend fold.  The fold computes
// (1 - sigmoid(p)) * branch + sigmoid(p) * other with other = x_s, so p is the mix factor NEGATED (sigmoid(-m) = 1 - sigmoid(m)).
//
// One clip per pass (a clip's pixels are bit-identical whatever else is in the call).  The fp32 stream of the whole clip is frame-major
// [F][h * w][C] in two ping-pong buffers (split fp16 mirrors where VaeStreams writes them); a third clip-sized buffer holds the temporal
// block's conv1 output, whose clip-wide statistics need every frame before any frame is normalised.  Launches run over groups of g
// consecutive frames: the spatial ResNets and up-sampler convs with N = g; a temporal conv as IG_TEMPORAL with t_pad = 1 on a padded
// split operand [g + 2][h * w][2 C] that op_gn_apply fills with frames [f0 - 1, f1 + 1) of the clip (zero slots at the clip's ends).
// g is the largest group whose operands obey the image decoder's index rule (below 2^31 elements), or the caller's cap.
#include "plan_vae_common.h"
#include <cmath>

namespace {

struct STResW {                  // SpatioTemporalResBlock (merge strategy learned, switch_spatial_to_temporal_mix)
    ResnetW sp;                  // spatial_res_block
    Norm tn1, tn2;               // temporal_res_block (C -> C, no shortcut, no temb)
    ConvW tc1, tc2;
    float* mix = nullptr;        // -time_mixer.mix_factor
};

struct TLevel {
    std::vector<STResW> res;
    bool resample = false;
    ConvW conv;
};

struct VaeTDecoder : StandalonePlan {
    ctrl_vae_decoder_config cfg{};
    float* wpq = nullptr;         // identity [lat][lat] and zero bias: the head kernel's post_quant_conv operands
    float* bpq = nullptr;
    ConvD conv_in;
    std::vector<STResW> mid;      // MidBlockTemporalDecoder: num_layers = layers_per_block ResNets, ONE attention
    Norm attn_gn;
    Lin qkv, attn_out;
    std::vector<TLevel> levels;
    Norm norm_out;
    ConvD conv_out;
    float* tw = nullptr;          // time_conv_out.weight fp32 [oc][oc][3]
    float* tb = nullptr;
    std::vector<float*> mixes;    // every STResW::mix (negated once after packing)
};

constexpr float kTemporalEps = 1e-5f;

int validate(const ctrl_vae_decoder_config& c) {
    TRY(validate_vae(c, "vae temporal decoder"));
    CTRL_CHECK(c.out_channels >= 1 && c.out_channels <= 4, "vae temporal decoder: out_channels must be 1 .. 4");
    return 0;
}

int build_st_res(ParamSink& ps, VaeTDecoder& t, const std::string& pre, int Cin, int Cout, STResW* w) {
    TRY(build_resnet(ps, pre + ".spatial_res_block", Cin, Cout, false, &w->sp, true));
    const std::string tp = pre + ".temporal_res_block";
    TRY(ps.norm(tp + ".norm1", Cout, &w->tn1));
    TRY(ps.conv(tp + ".conv1", Cout, Cout, 3, /*temporal*/ true, &w->tc1, /*dup*/ true));
    TRY(ps.norm(tp + ".norm2", Cout, &w->tn2));
    TRY(ps.conv(tp + ".conv2", Cout, Cout, 3, true, &w->tc2, true));
    TRY(ps.scalar(pre + ".time_mixer.mix_factor", &w->mix));
    if (w->mix) t.mixes.push_back(w->mix);
    return 0;
}

int build_tdec(ParamSink& ps, VaeTDecoder& t) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels, lat = c.latent_channels, Ct = c.block_out_channels[nl - 1], oc = c.out_channels;
    t.mixes.clear();
    TRY(ps.conv_direct("decoder.conv_in", Ct, lat, &t.conv_in));
    t.mid.resize(c.layers_per_block);
    TRY(build_st_res(ps, t, "decoder.mid_block.resnets.0", Ct, Ct, &t.mid[0]));
    const std::string ap = "decoder.mid_block.attentions.0.";
    TRY(ps.norm(ap + "group_norm", Ct, &t.attn_gn));
    TRY(ps.linear_cat({ap + "to_q", ap + "to_k", ap + "to_v"}, {Ct, Ct, Ct}, Ct, true, &t.qkv));
    TRY(ps.linear(ap + "to_out.0", Ct, Ct, true, false, &t.attn_out));
    for (int j = 1; j < c.layers_per_block; ++j) TRY(build_st_res(ps, t, "decoder.mid_block.resnets." + std::to_string(j), Ct, Ct, &t.mid[j]));
    t.levels.resize(nl);
    int cin = Ct;
    for (int i = 0; i < nl; ++i) {
        TLevel& lv = t.levels[i];
        const std::string pre = "decoder.up_blocks." + std::to_string(i) + ".";
        const int cout = c.block_out_channels[nl - 1 - i];
        lv.res.resize(c.layers_per_block + 1);
        for (int j = 0; j <= c.layers_per_block; ++j) {
            TRY(build_st_res(ps, t, pre + "resnets." + std::to_string(j), cin, cout, &lv.res[j]));
            cin = cout;
        }
        lv.resample = i + 1 < nl;
        if (lv.resample) TRY(ps.conv(pre + "upsamplers.0.conv", cout, cout, 3, false, &lv.conv, true));
    }
    TRY(ps.norm("decoder.conv_norm_out", cin, &t.norm_out));
    TRY(ps.conv_direct("decoder.conv_out", oc, cin, &t.conv_out));
    TRY(ps.raw_f32("decoder.time_conv_out.weight", {oc, oc, 3, 1, 1}, &t.tw));
    TRY(ps.raw_f32("decoder.time_conv_out.bias", {oc}, &t.tb));
    return 0;
}

// after packing: the mix factors negated in place, the identity post_quant_conv (plan creation only: synchronous copies)
int finish_build(VaeTDecoder& t, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    for (float* m : t.mixes) {
        float v = 0.f;
        HIP_TRY(hipMemcpy(&v, m, sizeof(float), hipMemcpyDeviceToHost));
        v = -v;
        HIP_TRY(hipMemcpy(m, &v, sizeof(float), hipMemcpyHostToDevice));
    }
    const int lat = t.cfg.latent_channels;
    std::vector<float> eye((size_t)lat * lat, 0.f), zero((size_t)lat, 0.f);
    for (int i = 0; i < lat; ++i) eye[(size_t)i * lat + i] = 1.f;
    TRY(t.pk->dalloc(eye.size() * sizeof(float), (void**)&t.wpq));
    TRY(t.pk->dalloc(zero.size() * sizeof(float), (void**)&t.bpq));
    HIP_TRY(hipMemcpy(t.wpq, eye.data(), eye.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.bpq, zero.data(), zero.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int collect(const ctrl_vae_decoder_config& c, SpecCollector& sc) {
    TRY(validate(c));
    VaeTDecoder t;
    t.cfg = c;
    return build_tdec(sc, t);
}

struct TDecFwd {
    const void* z; int zdt; int F, h, w;
    long img_stride, ch_stride;
    float scale; int kind;
    void* out; int odt;
    int g;                              // frames per launch
};

// frames [f0, ...) of a frame-major clip tensor [F][rows][C] (the split mirror rows are 2 C wide)
TV frames_from(const TV& x, int f0, size_t rows, int C) {
    TV v = x;
    v.p = (char*)x.p + (size_t)f0 * rows * C * sizeof(float);
    if (x.m16) v.m16 = x.m16 + (size_t)f0 * rows * C * (x.lo_off ? 2 : 1);
    return v;
}

// one temporal conv of frames [f0, f1): GroupNorm (the clip's statistics `st`) + SiLU of frames [f0 - 1, f1 + 1) of src into the padded
// split operand `pad` [g + 2][HW][2 C], zero slots outside the clip, then the IG_TEMPORAL GEMM of the f1 - f0 frames
int run_temporal_conv(Ctx& cx, const Norm& n, const ConvW& cw, const float* st, const TV& src, half_t* pad, int F, int f0, int f1, int HW,
                      IGemmArgs g /* outputs, residual and blend set by the caller */) {
    const int C = n.C, gf = f1 - f0;
    const int lo = std::max(f0 - 1, 0), hi = std::min(f1 + 1, F);
    const size_t slot = (size_t)HW * 2 * C;                    // halves per frame slot
    RUN(cx, op_gn_apply((const float*)src.p + (size_t)lo * HW * C, DT_F32, st, n.g, n.b, pad, 1, (hi - lo) * HW, C, 32, kTemporalEps, 1, cx.s,
                        2 * C, C, (long)F * HW, (long)(gf + 2) * HW, (long)(lo - (f0 - 1)) * HW));
    if (f0 == 0) RUN(cx, op_fill_zero(pad, slot * sizeof(half_t), cx.s));
    if (f1 == F) RUN(cx, op_fill_zero(pad + (size_t)(gf + 1) * slot, slot * sizeof(half_t), cx.s));
    g.A = pad; g.lda = 2 * C; g.mode = IG_TEMPORAL; g.Cin = cw.Cin; g.taps = 3; g.F = gf; g.HW = HW; g.t_pad = 1;
    g.W = cw.w; g.M = gf * HW; g.Nout = C; g.Ktot = 3 * cw.Cin; g.bias = cw.b; g.rows_per_img = HW; g.scale = 1.f; g.a_split = 1;
    RUN(cx, op_igemm(g, cx.s));
    return 0;
}

// x <- SpatioTemporalResBlock(x) over the clip's F frames at h x w, in groups of a.g frames; h1: the clip-sized conv1 buffer
int run_st_res(Ctx& cx, VaeStreams& st, const STResW& w, const TDecFwd& a, TV* x, bool need16, float* h1, int h, int wd, float eps) {
    const int F = a.F, HW = h * wd, C = w.sp.Cout, Cin = w.sp.Cin;
    CTRL_CHECK(w.tc1.dup && !w.tc1.paired && w.tc1.Cin == 2 * C && w.tc2.dup && !w.tc2.paired, "vae temporal decoder: the temporal convs "
                                                                                                  "take the weights-packed-twice form");
    TV xs = st.next(false, C);                                   // x_spatial
    for (int f0 = 0; f0 < F; f0 += a.g) {
        const int n = std::min(a.g, F - f0);
        TRY(run_resnet(cx, w.sp, frames_from(*x, f0, HW, Cin), frames_from(xs, f0, HW, C), n, h, wd, 1, nullptr, 0, eps));
    }
    TV out = st.next(need16, C);                                 // (the buffer x was in: every frame of x has been consumed)
    const size_t mk = cx.mark();
    half_t* pad = cx.h((size_t)(std::min(a.g, F) + 2) * HW * 2 * C);
    TV h1v; h1v.p = h1; h1v.dt = DT_F32;
    float* s1 = cx.stats(op_gn_stats_floats(1, F * HW, C, 32));
    RUN(cx, op_gn_stats(xs.p, DT_F32, s1, 1, F * HW, C, 32, cx.s));
    for (int f0 = 0; f0 < F; f0 += a.g) {
        const int f1 = std::min(F, f0 + a.g);
        IGemmArgs g = {};
        set_out(g, frames_from(h1v, f0, HW, C), C, C);
        TRY(run_temporal_conv(cx, w.tn1, w.tc1, s1, xs, pad, F, f0, f1, HW, g));
    }
    float* s2 = cx.stats(op_gn_stats_floats(1, F * HW, C, 32));
    RUN(cx, op_gn_stats(h1, DT_F32, s2, 1, F * HW, C, 32, cx.s));
    for (int f0 = 0; f0 < F; f0 += a.g) {
        const int f1 = std::min(F, f0 + a.g);
        const TV xsf = frames_from(xs, f0, HW, C);
        IGemmArgs g = {};
        set_res(g, xsf, C);
        set_out(g, frames_from(out, f0, HW, C), C, C);
        set_blend(g, w.mix, xsf, C);
        TRY(run_temporal_conv(cx, w.tn2, w.tc2, s2, h1v, pad, F, f0, f1, HW, g));
    }
    cx.release(mk);
    *x = out;
    return 0;
}

// one clip through the decoder
int run_clip(Ctx& cx, const VaeTDecoder& t, const TDecFwd& a, int clip) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels, lat = c.latent_channels, Ct = c.block_out_channels[nl - 1], F = a.F;
    const float eps = c.norm_eps;
    cx.stats_off = 0;
    TRY(begin_forward(cx));
    // per frame: the largest fp32 map of any level, and the largest map that is read as a convolution operand (its split mirror)
    size_t max32 = (size_t)a.h * a.w * Ct, max16 = 0;
    {
        int cin = Ct;
        size_t hw = (size_t)a.h * a.w;
        for (int i = 0; i < nl; ++i) {
            const TLevel& lv = t.levels[i];
            const int cout = lv.res[0].sp.Cout;
            max32 = std::max(max32, hw * std::max(cin, cout));
            if (lv.res[0].sp.has_shortcut) max16 = std::max(max16, hw * cin);
            if (lv.resample) { max16 = std::max(max16, hw * cout); hw *= 4; max32 = std::max(max32, hw * cout); }
            cin = cout;
        }
    }
    VaeStreams streams(cx, (size_t)F * max32, (size_t)F * max16);
    float* h1 = cx.f((size_t)F * max32);
    int h = a.h, w = a.w;
    const size_t zsz = dt_size(a.zdt);
    for (int f = 0; f < F; ++f) {
        const char* z = (const char*)a.z + ((size_t)clip * F + f) * a.img_stride * zsz;
        RUN(cx, op_vae_dec_head(z, a.zdt, a.scale, t.wpq, t.bpq, t.conv_in.w, t.conv_in.b, streams.s32[0] + (size_t)f * h * w * Ct, lat, h, w,
                                a.ch_stride, Ct, cx.s));
    }
    TV x = streams.first();
    // diffusers runs resnets[0], then zip(resnets[1:], attentions): with its one attention that is (attention, resnets[1]) when
    // layers_per_block >= 2 and nothing more (further ResNets are parameters only)
    const bool mid_attn = t.mid.size() >= 2, need16_mid = t.levels[0].res[0].sp.has_shortcut;
    TRY(run_st_res(cx, streams, t.mid[0], a, &x, mid_attn ? false : need16_mid, h1, h, w, eps));
    if (mid_attn) {
        TV y = streams.next(false, Ct);
        for (int f = 0; f < F; ++f)
            TRY(run_vae_mid_attention(cx, t.attn_gn, t.qkv, t.attn_out, Ct, eps, frames_from(x, f, (size_t)h * w, Ct),
                                      frames_from(y, f, (size_t)h * w, Ct), h * w));
        x = y;
        TRY(run_st_res(cx, streams, t.mid[1], a, &x, need16_mid, h1, h, w, eps));
    }
    ConvOpts up; up.up = 2;                    // nearest x2 in the gather
    for (int i = 0; i < nl; ++i) {
        const TLevel& lv = t.levels[i];
        const int n = (int)lv.res.size(), C = lv.res.back().sp.Cout;
        for (int j = 0; j < n; ++j)
            TRY(run_st_res(cx, streams, lv.res[j], a, &x, j + 1 < n ? lv.res[j + 1].sp.has_shortcut : lv.resample, h1, h, w, eps));
        if (lv.resample) {
            TV y = streams.next(t.levels[i + 1].res[0].sp.has_shortcut, C);
            for (int f0 = 0; f0 < F; f0 += a.g) {
                const int nf = std::min(a.g, F - f0);
                TRY(run_conv(cx, lv.conv, frames_from(x, f0, (size_t)h * w, C).m16, frames_from(y, f0, (size_t)4 * h * w, C), nf, h, w, up));
            }
            x = y;
            h *= 2; w *= 2;
        }
    }
    const int C0 = t.norm_out.C, oc = c.out_channels;
    const size_t HW = (size_t)h * w;
    float* frames = cx.f((size_t)F * oc * HW);                   // conv_out's fp32 NCHW frames
    for (int f = 0; f < F; ++f) {
        const float* xf = (const float*)x.p + (size_t)f * HW * C0;
        float* st = cx.stats(op_gn_stats_floats(1, h * w, C0, 32));
        RUN(cx, op_gn_stats(xf, DT_F32, st, 1, h * w, C0, 32, cx.s));
        RUN(cx, op_vae_dec_tail(xf, st, t.norm_out.g, t.norm_out.b, eps, t.conv_out.w, t.conv_out.b, h, w, C0, oc, CTRL_VAE_DEC_SAMPLE,
                                frames + (size_t)f * oc * HW, DT_F32, cx.s));
    }
    const size_t per = (size_t)oc * HW * (a.kind == CTRL_VAE_DEC_SAMPLE ? dt_size(a.odt) : (a.kind == CTRL_VAE_DEC_UNIT ? 4 : 1));
    RUN(cx, op_vae_time_conv(frames, t.tw, t.tb, F, h, w, oc, a.kind, (char*)a.out + (size_t)clip * F * per, a.odt, cx.s));
    return 0;
}

// the largest group of frames (<= cap) whose launches keep every operand below 2^31 elements: the padded split operand of the temporal
// convs, (g + 2) * HW * 2 * C, and the split GroupNorm output of the widest ResNet / up-sampler input, g * HW * 2 * max(cin, cout)
// (the image decoder's rule over g frames); 0: not even one frame fits
int frames_per_launch(const ctrl_vae_decoder_config& c, int h, int w, int cap) {
    const int nl = c.num_levels;
    double g = cap;
    int cin = c.block_out_channels[nl - 1];
    double hw = (double)h * w;
    const double lim = 2147483648.0;
    for (int i = 0; i < nl; ++i) {
        const int cout = c.block_out_channels[nl - 1 - i];
        const double gs = std::ceil(lim / (hw * 2.0 * std::max(cin, cout))) - 1.0;       // largest g with g * x < lim
        const double gt = std::ceil(lim / (hw * 2.0 * cout)) - 1.0 - 2.0;
        g = std::min(g, std::min(gs, gt));
        cin = cout;
        if (i + 1 < nl) hw *= 4.0;
    }
    return g < 1.0 ? 0 : (int)g;
}

int forward(VaeTDecoder& t, TDecFwd a, int clips, int fpl, hipStream_t s) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels;
    CTRL_CHECK(a.z != nullptr && a.out != nullptr, "vae temporal decoder: latents and out are required");
    CTRL_CHECK(a.zdt == DT_F32 || a.zdt == DT_F16 || a.zdt == DT_BF16, "vae temporal decoder: latent dtype must be fp32, fp16 or bf16 (NCHW)");
    CTRL_CHECK(clips >= 1 && a.F >= 1 && a.F <= 4096, "vae temporal decoder: clips and num_frames must be positive (at most 4096 frames)");
    CTRL_CHECK(fpl >= 0, "vae temporal decoder: frames_per_launch must be 0 (the largest group) or positive");
    CTRL_CHECK(a.h >= 1 && a.w >= 1 && ((long)a.h << (nl - 1)) <= 4096 && ((long)a.w << (nl - 1)) <= 4096,
               "vae temporal decoder: the image (latent size * 2^(levels-1)) must be at most 4096 on a side");
    CTRL_CHECK((long)a.h * a.w <= 65536, "vae temporal decoder: at most 65536 latent positions (the mid-block attention's sequence)");
    CTRL_CHECK(a.ch_stride >= (long)a.h * a.w && a.img_stride >= 0,
               "vae temporal decoder: the channel stride must be at least h * w elements (dense [h][w] planes) and the image stride not negative");
    a.g = frames_per_launch(c, a.h, a.w, fpl > 0 ? std::min(fpl, a.F) : a.F);
    CTRL_CHECK(a.g >= 1, "vae temporal decoder: the image is too large: a level's split operand (pixels x 2 x channels, three frames of it "
                         "for a temporal convolution) must stay below 2^31 elements -- decode in tiles");
    // the clip-wide GroupNorm walks F * H * W rows with int row counts
    CTRL_CHECK((double)a.F * a.h * a.w * std::pow(4.0, nl - 1) < 2147483648.0, "vae temporal decoder: the clip (frames x pixels) must stay below 2^31 rows");
    CTRL_CHECK(a.kind == CTRL_VAE_DEC_SAMPLE || a.kind == CTRL_VAE_DEC_UNIT || a.kind == CTRL_VAE_DEC_U8, "vae temporal decoder: kind must be 0, 1 or 2");
    CTRL_CHECK(a.odt == DT_F32 || a.odt == DT_F16 || a.odt == DT_BF16, "vae temporal decoder: out_dtype must be fp32, fp16 or bf16");
    return run_per_image(t, clips, s, "vae temporal decoder", [&](Ctx& cx, int n) { return run_clip(cx, t, a, n); });
}

}  // namespace

extern "C" {

int ctrl_vae_tdecoder_param_count(const ctrl_vae_decoder_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_vae_tdecoder_param_spec(const ctrl_vae_decoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "vae_tdecoder_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "vae_tdecoder_param_spec", name, name_len, shape, ndim);
}

int ctrl_vae_tdecoder_create(const ctrl_vae_decoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                             ctrl_vae_tdecoder** out) {
    return plan_create<VaeTDecoder>("vae_tdecoder_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_tdec, finish_build);
}

void ctrl_vae_tdecoder_destroy(ctrl_vae_tdecoder* h) { plan_destroy<VaeTDecoder>(h); }

int ctrl_vae_tdecoder_forward(ctrl_vae_tdecoder* h, const void* latents, int latent_dtype, int clips, int num_frames, int lat_h, int lat_w,
                              int64_t image_stride, int64_t channel_stride, float scale, int kind, void* out, int out_dtype,
                              int frames_per_launch, void* stream) {
    CTRL_CHECK(h != nullptr, "vae_tdecoder_forward: null plan");
    VaeTDecoder* t = (VaeTDecoder*)h;
    DeviceGuard dg(t->device);
    const TDecFwd a = {latents, latent_dtype, num_frames, lat_h, lat_w, (long)image_stride, (long)channel_stride, scale, kind, out, out_dtype, 0};
    return forward(*t, a, clips, frames_per_launch, S(stream));
}

int ctrl_op_vae_time_conv(const float* x, const float* w, const float* b, int F, int H, int W, int Cout, int kind, void* out,
                          int out_dtype, void* stream) {
    return op_vae_time_conv(x, w, b, F, H, W, Cout, kind, out, out_dtype, S(stream));
}

}  // extern "C"
