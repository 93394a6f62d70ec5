// KL-VAE encoder plan (diffusers v0.27 Encoder + quant_conv + DiagonalGaussianDistribution, the encoder half of AutoencoderKL and of
// SVD's AutoencoderKLTemporalDecoder: the SVD pipeline's _encode_vae_image, svd/pipelines/svd_controlnet_adapter_pipeline.py:214-235,
// and I2VGen-XL's prepare_image_latents, i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:487-518):
//   conv_in (direct 3 -> C0 conv on the NCHW pixels, any dtype, fp32 out) | per level: ResnetBlock2D x layers (no temb) + Downsample2D on all but
//   the last level (F.pad(0, 1, 0, 1) + stride-2 3x3 conv = the implicit GEMM with tap_origin 1) | mid block: ResNet, attention (own
//   GroupNorm; ONE head of dim C: S = Q K^T / sqrt(C) on the GEMM in fp32, the fp32 row softmax of vae.hip, O = P V on the GEMM, in
//   query-row chunks whose S | P workspace stays under 256 MB: run_vae_mid_attention, plan_common.cpp), to_out + residual, ResNet | conv_norm_out + SiLU | conv_out (weights
//   padded to 16 output rows) | the posterior kernel (quant_conv, clamp, mode / sample / moments).
// The residual stream is fp32 from conv_in on.  Every convolution reads a split [hi | lo] fp16 operand (ctrl_igemm_desc::a_split): the
// GroupNorm + SiLU outputs, and the stream's split mirror for the shortcut and downsample convolutions.  Plain fp16 operands measured
// 2.6e-3 rel-inf at 512^2, over the 1e-3 bound; the attention's Q / K / V / P stay fp16 (1.1e-4 of the error, fp32 restatement with
// only those rounded).  Images run one after the other through the same launches (M = one image's pixels): an
// image's latents are bit-identical whatever the batch.  The first forward at a larger image size allocates the workspace; every later
// forward allocates nothing and is capturable.
#include "plan_vae_common.h"
#include <cmath>

namespace {

constexpr int kConvOutRows = 16;            // conv_out's weight rows padded to one MFMA tile column block

struct VaeEncoder : StandalonePlan {
    ctrl_vae_encoder_config cfg{};
    ConvD conv_in;
    std::vector<VaeLevel> levels;
    VaeMid mid;
    Norm norm_out;
    ConvW conv_out, conv_out16;   // conv_out16: the 2*lat rows of conv_out padded to kConvOutRows (zero rows, zero bias)
    float* wq = nullptr;          // quant_conv.weight fp32 [2lat][2lat]
    float* bq = nullptr;
};

int validate(const ctrl_vae_encoder_config& c) { return validate_vae(c, "vae encoder"); }

int build_vae(ParamSink& ps, VaeEncoder& t) {
    const ctrl_vae_encoder_config& c = t.cfg;
    const int nl = c.num_levels, lat2 = 2 * c.latent_channels, Ct = c.block_out_channels[nl - 1];
    TRY(ps.conv_direct("encoder.conv_in", c.block_out_channels[0], 3, &t.conv_in));
    t.levels.resize(nl);
    int cin = c.block_out_channels[0];
    for (int i = 0; i < nl; ++i)
        TRY(build_vae_level(ps, "encoder.down_blocks." + std::to_string(i) + ".", c.layers_per_block, &cin, c.block_out_channels[i],
                            i + 1 < nl, "downsamplers.0.conv", &t.levels[i]));
    TRY(build_vae_mid(ps, "encoder.", Ct, &t.mid));
    TRY(ps.norm("encoder.conv_norm_out", Ct, &t.norm_out));
    TRY(ps.conv("encoder.conv_out", lat2, Ct, 3, false, &t.conv_out, true));
    TRY(ps.raw_f32("quant_conv.weight", {lat2, lat2, 1, 1}, &t.wq));
    TRY(ps.raw_f32("quant_conv.bias", {lat2}, &t.bq));
    return 0;
}

int collect(const ctrl_vae_encoder_config& c, SpecCollector& sc) {
    TRY(validate(c));
    VaeEncoder t;
    t.cfg = c;
    return build_vae(sc, t);
}

// conv_out with its weight rows padded to kConvOutRows (the packed layout [Cout][9][Cin] keeps a row per output channel; Cin per tap is
// the logical width for the paired split walk, twice it for the duplicated pack)
int pad_conv_out(VaeEncoder& t, hipStream_t s) {
    const ConvW& c = t.conv_out;
    ConvW& p = t.conv_out16;
    p = c;
    p.Cout = kConvOutRows;
    const size_t row = (size_t)c.taps * (c.paired ? c.Cin / 2 : c.Cin) * sizeof(half_t);
    TRY(t.pk->dalloc(row * kConvOutRows, (void**)&p.w));
    TRY(t.pk->dalloc(kConvOutRows * sizeof(float), (void**)&p.b));
    HIP_TRY(hipMemsetAsync(p.w, 0, row * kConvOutRows, s));
    HIP_TRY(hipMemsetAsync(p.b, 0, kConvOutRows * sizeof(float), s));
    HIP_TRY(hipMemcpyAsync(p.w, c.w, row * c.Cout, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(p.b, c.b, c.Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

struct VaeFwd {
    const void* px; int pdt; int H, W;
    const void* eps; int eps_dt; float scale; int kind;
    void* out; int odt;
};

// one image through the encoder: pixels of image n -> its latents
int run_image(Ctx& cx, const VaeEncoder& t, const VaeFwd& a, int n) {
    const ctrl_vae_encoder_config& c = t.cfg;
    const int nl = c.num_levels, lat = c.latent_channels, H = a.H, W = a.W;
    const float eps = c.norm_eps;
    cx.stats_off = 0;
    TRY(begin_forward(cx));
    // the two stream buffers (fp32 + split fp16 mirror each) hold the largest map of any level
    size_t maxe = (size_t)H * W * c.block_out_channels[0];
    for (int i = 0; i < nl; ++i) maxe = std::max(maxe, ((size_t)H >> i) * ((size_t)W >> i) * c.block_out_channels[i]);
    VaeStreams streams(cx, maxe, maxe);
    const int C0 = c.block_out_channels[0];
    const char* px = (const char*)a.px + (size_t)n * 3 * H * W * dt_size(a.pdt);
    RUN(cx, op_vae_conv_in(px, a.pdt, t.conv_in.w, t.conv_in.b, streams.s32[0], H, W, C0, cx.s));
    TV x = streams.first();
    int h = H, w = W;
    ConvOpts down; down.stride = 2; down.tap_origin = 1;
    for (int i = 0; i < nl; ++i) {
        TRY(run_vae_level(cx, streams, t.levels[i], down, i + 1 < nl && t.levels[i + 1].res[0].has_shortcut, &x, h, w, eps));
        if (t.levels[i].resample) { h /= 2; w /= 2; }
    }
    const int L = h * w;
    const int Ct = c.block_out_channels[nl - 1];
    TRY(run_vae_mid(cx, streams, t.mid, &x, false, h, w, eps));
    half_t* g16 = cx.h((size_t)L * 2 * Ct);
    TRY(run_groupnorm(cx, t.norm_out, x, g16, 1, L, eps, true, true));
    TV co; co.p = cx.f((size_t)L * kConvOutRows); co.dt = DT_F32;
    TRY(run_conv(cx, t.conv_out16, g16, co, 1, h, w, ConvOpts()));
    const size_t per = (size_t)(a.kind == CTRL_VAE_MOMENTS ? 4 : 1) * lat * L;
    const void* e = a.eps ? (const char*)a.eps + (size_t)n * lat * L * dt_size(a.eps_dt) : nullptr;
    void* o = (char*)a.out + (size_t)n * per * dt_size(a.odt);
    RUN(cx, op_vae_posterior((const float*)co.p, kConvOutRows, 0, t.wq, t.bq, 1, lat, h, w, e, a.eps_dt, a.scale, a.kind, o, a.odt, cx.s));
    return 0;
}

int forward(VaeEncoder& t, const VaeFwd& a, int N, hipStream_t s) {
    const ctrl_vae_encoder_config& c = t.cfg;
    const int f = 1 << (c.num_levels - 1);
    CTRL_CHECK(a.px != nullptr && a.out != nullptr, "vae encoder: pixels and out are required");
    CTRL_CHECK(a.pdt == DT_F32 || a.pdt == DT_F16 || a.pdt == DT_BF16, "vae encoder: pixel dtype must be fp32, fp16 or bf16 (NCHW)");
    CTRL_CHECK(N >= 1, "vae encoder: N must be positive");
    CTRL_CHECK(a.H >= 8 && a.W >= 8 && a.H % 8 == 0 && a.W % 8 == 0 && a.H % f == 0 && a.W % f == 0 && a.H <= 4096 && a.W <= 4096,
               "vae encoder: H and W must be multiples of 8 and of 2^(levels-1), at most 4096");
    CTRL_CHECK(a.kind == CTRL_VAE_MODE || a.kind == CTRL_VAE_SAMPLE || a.kind == CTRL_VAE_MOMENTS, "vae encoder: kind must be 0, 1 or 2");
    CTRL_CHECK(a.kind != CTRL_VAE_SAMPLE || (a.eps && (a.eps_dt == DT_F32 || a.eps_dt == DT_F16 || a.eps_dt == DT_BF16)),
               "vae encoder: sampling needs eps in fp32, fp16 or bf16");
    CTRL_CHECK(a.odt == DT_F32 || a.odt == DT_F16 || a.odt == DT_BF16, "vae encoder: out_dtype must be fp32, fp16 or bf16");
    return run_per_image(t, N, s, "vae encoder", [&](Ctx& cx, int n) { return run_image(cx, t, a, n); });
}

}  // namespace

extern "C" {

int ctrl_vae_encoder_param_count(const ctrl_vae_encoder_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_vae_encoder_param_spec(const ctrl_vae_encoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "vae_encoder_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "vae_encoder_param_spec", name, name_len, shape, ndim);
}

int ctrl_vae_encoder_create(const ctrl_vae_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                            ctrl_vae_encoder** out) {
    return plan_create<VaeEncoder>("vae_encoder_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_vae, pad_conv_out);
}

void ctrl_vae_encoder_destroy(ctrl_vae_encoder* h) { plan_destroy<VaeEncoder>(h); }

int ctrl_vae_encoder_forward(ctrl_vae_encoder* h, const void* pixels, int pixel_dtype, int N, int H, int W, const void* eps, int eps_dtype,
                             float scale, int kind, void* out, int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "vae_encoder_forward: null plan");
    VaeEncoder* t = (VaeEncoder*)h;
    DeviceGuard dg(t->device);
    const VaeFwd a = {pixels, pixel_dtype, H, W, eps, eps_dtype, scale, kind, out, out_dtype};
    return forward(*t, a, N, S(stream));
}

int ctrl_op_vae_row_softmax(const float* scores, int64_t lds, void* P, int64_t ldp, int rows, int L, int Lpad, void* stream) {
    return op_vae_row_softmax(scores, lds, (half_t*)P, ldp, rows, L, Lpad, S(stream));
}

int ctrl_op_vae_posterior(const float* x, int64_t ldx, int x_nchw, const float* wq, const float* bq, int N, int lat, int h, int w,
                          const void* eps, int eps_dtype, float scale, int kind, void* out, int out_dtype, void* stream) {
    return op_vae_posterior(x, ldx, x_nchw, wq, bq, N, lat, h, w, eps, eps_dtype, scale, kind, out, out_dtype, S(stream));
}

}  // extern "C"
