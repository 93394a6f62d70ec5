// KL-VAE decoder plan (diffusers v0.27 AutoencoderKL.decode = post_quant_conv + Decoder: the image decode of the SDXL pipeline,
// sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1406-1427, and I2VGen-XL's decode_latents,
// i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:398-418):
//   head kernel (latents * scale -> post_quant_conv -> conv_in, fp32, vae.hip) | mid block: ResNet, attention (run_vae_mid_attention, the
//   encoder's), ResNet | per level over the reversed block_out_channels: layers_per_block + 1 ResNets (no temb) + Upsample2D on all but the
//   last level (nearest x2 + 3x3 conv = the implicit GEMM's up = 2 gather on the stream's split mirror) | the GroupNorm statistics pass over
//   the last stream | tail kernel (conv_norm_out + SiLU + conv_out + the output epilogue in one pass, fp32, vae.hip).
// As in the encoder plan (plan_vae.cpp) the residual stream is fp32 from conv_in on, every implicit-GEMM convolution reads a split
// [hi | lo] fp16 operand, the attention's Q / K / V / P are fp16, and images run one after the other through the same launches (an image's
// pixels are bit-identical whatever the batch).  conv_out's input never leaves fp32.  The first forward at a larger latent size allocates
// the workspace; every later forward allocates nothing and is capturable.
#include "plan_vae_common.h"

namespace {

struct VaeDecoder : StandalonePlan {
    ctrl_vae_decoder_config cfg{};
    float* wpq = nullptr;         // post_quant_conv.weight fp32 [lat][lat]
    float* bpq = nullptr;
    ConvD conv_in;                // fp32 [9][lat][C_top]
    VaeMid mid;
    Norm norm_out;
    std::vector<VaeLevel> levels;
    ConvD conv_out;               // fp32 [9][C0][out_channels]
};

int validate(const ctrl_vae_decoder_config& c) {
    TRY(validate_vae(c, "vae decoder"));
    CTRL_CHECK(c.out_channels >= 1 && c.out_channels <= 4, "vae decoder: out_channels must be 1 .. 4");
    return 0;
}

int build_dec(ParamSink& ps, VaeDecoder& t) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels, lat = c.latent_channels, Ct = c.block_out_channels[nl - 1];
    TRY(ps.raw_f32("post_quant_conv.weight", {lat, lat, 1, 1}, &t.wpq));
    TRY(ps.raw_f32("post_quant_conv.bias", {lat}, &t.bpq));
    TRY(ps.conv_direct("decoder.conv_in", Ct, lat, &t.conv_in));
    TRY(build_vae_mid(ps, "decoder.", Ct, &t.mid));
    t.levels.resize(nl);
    int cin = Ct;
    for (int i = 0; i < nl; ++i)
        TRY(build_vae_level(ps, "decoder.up_blocks." + std::to_string(i) + ".", c.layers_per_block + 1, &cin, c.block_out_channels[nl - 1 - i],
                            i + 1 < nl, "upsamplers.0.conv", &t.levels[i]));
    TRY(ps.norm("decoder.conv_norm_out", cin, &t.norm_out));
    TRY(ps.conv_direct("decoder.conv_out", c.out_channels, cin, &t.conv_out));
    return 0;
}

int collect(const ctrl_vae_decoder_config& c, SpecCollector& sc) {
    TRY(validate(c));
    VaeDecoder t;
    t.cfg = c;
    return build_dec(sc, t);
}

struct DecFwd {
    const void* z; int zdt; int h, w;
    long img_stride, ch_stride;        // elements between the images and between an image's dense [h][w] channel planes
    float scale; int kind;
    void* out; int odt;
};

// one image through the decoder: latents of image n -> its pixels
int run_image(Ctx& cx, const VaeDecoder& t, const DecFwd& a, int n) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels, lat = c.latent_channels, Ct = c.block_out_channels[nl - 1];
    const float eps = c.norm_eps;
    cx.stats_off = 0;
    TRY(begin_forward(cx));
    // the two stream buffers hold the largest map of any level (fp32), and the largest map that is read as a convolution operand
    // (its split fp16 mirror: 2 x the channels)
    size_t max32 = (size_t)a.h * a.w * Ct, max16 = 0;
    {
        int cin = Ct;
        size_t hw = (size_t)a.h * a.w;
        for (int i = 0; i < nl; ++i) {
            const VaeLevel& lv = t.levels[i];
            const int cout = lv.res[0].Cout;
            max32 = std::max(max32, hw * std::max(cin, cout));
            if (lv.res[0].has_shortcut) max16 = std::max(max16, hw * cin);
            if (lv.resample) { max16 = std::max(max16, hw * cout); hw *= 4; max32 = std::max(max32, hw * cout); }
            cin = cout;
        }
    }
    VaeStreams streams(cx, max32, max16);
    int h = a.h, w = a.w;
    const char* z = (const char*)a.z + (size_t)n * a.img_stride * dt_size(a.zdt);
    RUN(cx, op_vae_dec_head(z, a.zdt, a.scale, t.wpq, t.bpq, t.conv_in.w, t.conv_in.b, streams.s32[0], lat, h, w, a.ch_stride, Ct, cx.s));
    TV x = streams.first();
    TRY(run_vae_mid(cx, streams, t.mid, &x, t.levels[0].res[0].has_shortcut, h, w, eps));
    ConvOpts up; up.up = 2;                    // nearest x2 in the gather
    for (int i = 0; i < nl; ++i) {
        TRY(run_vae_level(cx, streams, t.levels[i], up, i + 1 < nl && t.levels[i + 1].res[0].has_shortcut, &x, h, w, eps));
        if (t.levels[i].resample) { h *= 2; w *= 2; }
    }
    const int C0 = t.norm_out.C, oc = c.out_channels;
    float* st = cx.stats(op_gn_stats_floats(1, h * w, C0, 32));
    RUN(cx, op_gn_stats(x.p, x.dt, st, 1, h * w, C0, 32, cx.s));
    const size_t per = (size_t)oc * h * w * (a.kind == CTRL_VAE_DEC_SAMPLE ? dt_size(a.odt) : (a.kind == CTRL_VAE_DEC_UNIT ? 4 : 1));
    void* o = (char*)a.out + (size_t)n * per;
    RUN(cx, op_vae_dec_tail((const float*)x.p, st, t.norm_out.g, t.norm_out.b, eps, t.conv_out.w, t.conv_out.b, h, w, C0, oc, a.kind, o,
                            a.odt, cx.s));
    return 0;
}

int forward(VaeDecoder& t, const DecFwd& a, int N, hipStream_t s) {
    const ctrl_vae_decoder_config& c = t.cfg;
    const int nl = c.num_levels;
    CTRL_CHECK(a.z != nullptr && a.out != nullptr, "vae decoder: latents and out are required");
    CTRL_CHECK(a.zdt == DT_F32 || a.zdt == DT_F16 || a.zdt == DT_BF16, "vae decoder: latent dtype must be fp32, fp16 or bf16 (NCHW)");
    CTRL_CHECK(N >= 1, "vae decoder: N must be positive");
    CTRL_CHECK(a.h >= 1 && a.w >= 1 && ((long)a.h << (nl - 1)) <= 4096 && ((long)a.w << (nl - 1)) <= 4096,
               "vae decoder: the image (latent size * 2^(levels-1)) must be at most 4096 on a side");
    CTRL_CHECK((long)a.h * a.w <= 65536, "vae decoder: at most 65536 latent positions (the mid-block attention's sequence)");
    CTRL_CHECK(a.ch_stride >= (long)a.h * a.w && a.img_stride >= 0,
               "vae decoder: the channel stride must be at least h * w elements (dense [h][w] planes) and the image stride not negative");
    // index widths: the implicit GEMM's epilogue addresses the split mirror with 32-bit element offsets, its wide-tile gather with 32-bit
    // byte offsets (it steps aside above 2 GiB), GroupNorm, softmax and the head / tail kernels with 64-bit ones; the largest operand of a
    // level is the split GroupNorm output [rows][2 * C] of its widest ResNet input -- kept below 2^31 elements (2048^2 x 256 is exactly 2^31)
    {
        int cin = c.block_out_channels[nl - 1];
        double hw = (double)a.h * a.w;
        for (int i = 0; i < nl; ++i) {
            const int cout = c.block_out_channels[nl - 1 - i];
            CTRL_CHECK(hw * 2.0 * std::max(cin, cout) < 2147483648.0,
                       "vae decoder: the image is too large: a level's split operand (pixels x 2 x channels) must stay below 2^31 "
                       "elements -- decode in tiles");
            cin = cout;
            if (i + 1 < nl) hw *= 4.0;
        }
    }
    CTRL_CHECK(a.kind == CTRL_VAE_DEC_SAMPLE || a.kind == CTRL_VAE_DEC_UNIT || a.kind == CTRL_VAE_DEC_U8, "vae decoder: kind must be 0, 1 or 2");
    CTRL_CHECK(a.odt == DT_F32 || a.odt == DT_F16 || a.odt == DT_BF16, "vae decoder: out_dtype must be fp32, fp16 or bf16");
    return run_per_image(t, N, s, "vae decoder", [&](Ctx& cx, int n) { return run_image(cx, t, a, n); });
}

}  // namespace

extern "C" {

int ctrl_vae_decoder_param_count(const ctrl_vae_decoder_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_vae_decoder_param_spec(const ctrl_vae_decoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "vae_decoder_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "vae_decoder_param_spec", name, name_len, shape, ndim);
}

int ctrl_vae_decoder_create(const ctrl_vae_decoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                            ctrl_vae_decoder** out) {
    return plan_create<VaeDecoder>("vae_decoder_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_dec,
                                   [](VaeDecoder&, hipStream_t) { return 0; });
}

void ctrl_vae_decoder_destroy(ctrl_vae_decoder* h) { plan_destroy<VaeDecoder>(h); }

int ctrl_vae_decoder_forward_strided(ctrl_vae_decoder* h, const void* latents, int latent_dtype, int N, int lat_h, int lat_w,
                                     int64_t image_stride, int64_t channel_stride, float scale, int kind, void* out, int out_dtype,
                                     void* stream) {
    CTRL_CHECK(h != nullptr, "vae_decoder_forward: null plan");
    VaeDecoder* t = (VaeDecoder*)h;
    DeviceGuard dg(t->device);
    const DecFwd a = {latents, latent_dtype, lat_h, lat_w, (long)image_stride, (long)channel_stride, scale, kind, out, out_dtype};
    return forward(*t, a, N, S(stream));
}

int ctrl_vae_decoder_forward(ctrl_vae_decoder* h, const void* latents, int latent_dtype, int N, int lat_h, int lat_w, float scale, int kind,
                             void* out, int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "vae_decoder_forward: null plan");
    const int64_t plane = (int64_t)lat_h * lat_w;
    return ctrl_vae_decoder_forward_strided(h, latents, latent_dtype, N, lat_h, lat_w, plane * ((VaeDecoder*)h)->cfg.latent_channels, plane,
                                            scale, kind, out, out_dtype, stream);
}

int ctrl_op_vae_dec_head(const void* z, int z_dtype, float scale, const float* wpq, const float* bpq, const float* w_in, const float* b_in,
                         float* out, int lat, int h, int w, int64_t ch_stride, int Cout, void* stream) {
    return op_vae_dec_head(z, z_dtype, scale, wpq, bpq, w_in, b_in, out, lat, h, w, (long)ch_stride, Cout, S(stream));
}

int ctrl_op_vae_dec_tail(const float* x, const float* stats, const float* gamma, const float* beta, float eps, const float* w_out,
                         const float* b_out, int H, int W, int C, int Cout, int kind, void* out, int out_dtype, void* stream) {
    return op_vae_dec_tail(x, stats, gamma, beta, eps, w_out, b_out, H, W, C, Cout, kind, out, out_dtype, S(stream));
}

}  // extern "C"
