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
// image's latents are bit-identical whatever the batch.  The first forward of a larger image size allocates the workspace; every later
// forward allocates nothing and is capturable.
#include "plan_common.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kConvOutRows = 16;            // conv_out's weight rows padded to one MFMA tile column block

struct VaeLevel {
    std::vector<ResnetW> res;
    bool down = false;
    ConvW down_conv;
};

struct VaeEncoder : PlanBase {
    ctrl_vae_encoder_config cfg{};
    Packer* pk = nullptr;
    ConvD conv_in;
    std::vector<VaeLevel> levels;
    ResnetW mid0, mid1;
    Norm attn_gn, norm_out;
    Lin qkv, attn_out;
    ConvW conv_out, conv_out16;   // conv_out16: the 2*lat rows of conv_out padded to kConvOutRows (zero rows, zero bias)
    float* wq = nullptr;          // quant_conv.weight fp32 [2lat][2lat]
    float* bq = nullptr;
    Arena ar;
    ~VaeEncoder() {
        if (pk) { pk->release_all(); delete pk; }
    }
};

int validate(const ctrl_vae_encoder_config& c) {
    CTRL_CHECK(c.num_levels >= 1 && c.num_levels <= 4, "vae encoder: 1 to 4 levels (block_out_channels)");
    for (int i = 0; i < c.num_levels; ++i)
        CTRL_CHECK(c.block_out_channels[i] >= 32 && c.block_out_channels[i] <= 2048 && c.block_out_channels[i] % 32 == 0,
                   "vae encoder: block_out_channels must be multiples of 32 up to 2048");
    CTRL_CHECK(c.layers_per_block >= 1 && c.layers_per_block <= 8, "vae encoder: layers_per_block must be 1 .. 8");
    CTRL_CHECK(c.latent_channels >= 1 && c.latent_channels <= 8, "vae encoder: latent_channels must be 1 .. 8");
    CTRL_CHECK(c.norm_num_groups == 32, "vae encoder: norm_num_groups must be 32");
    CTRL_CHECK(c.norm_eps > 0.f, "vae encoder: norm_eps must be positive");
    return 0;
}

int build_vae(ParamSink& ps, VaeEncoder& t) {
    const ctrl_vae_encoder_config& c = t.cfg;
    const int nl = c.num_levels, lat2 = 2 * c.latent_channels, Ct = c.block_out_channels[nl - 1];
    TRY(ps.conv_direct("encoder.conv_in", c.block_out_channels[0], 3, &t.conv_in));
    t.levels.resize(nl);
    int cin = c.block_out_channels[0];
    for (int i = 0; i < nl; ++i) {
        const int cout = c.block_out_channels[i];
        VaeLevel& lv = t.levels[i];
        lv.res.resize(c.layers_per_block);
        const std::string pre = "encoder.down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block; ++j) {
            TRY(build_resnet(ps, pre + "resnets." + std::to_string(j), cin, cout, false, &lv.res[j], true));
            cin = cout;
        }
        lv.down = i + 1 < nl;
        if (lv.down) TRY(ps.conv(pre + "downsamplers.0.conv", cout, cout, 3, false, &lv.down_conv, true));
    }
    TRY(build_resnet(ps, "encoder.mid_block.resnets.0", Ct, Ct, false, &t.mid0, true));
    const std::string ap = "encoder.mid_block.attentions.0.";
    TRY(ps.norm(ap + "group_norm", Ct, &t.attn_gn));
    TRY(ps.linear_cat({ap + "to_q", ap + "to_k", ap + "to_v"}, {Ct, Ct, Ct}, Ct, true, &t.qkv));
    TRY(ps.linear(ap + "to_out.0", Ct, Ct, true, false, &t.attn_out));
    TRY(build_resnet(ps, "encoder.mid_block.resnets.1", Ct, Ct, false, &t.mid1, true));
    TRY(ps.norm("encoder.conv_norm_out", Ct, &t.norm_out));
    TRY(ps.conv("encoder.conv_out", lat2, Ct, 3, false, &t.conv_out, true));
    TRY(ps.raw_f32("quant_conv.weight", {lat2, lat2, 1, 1}, &t.wq));
    TRY(ps.raw_f32("quant_conv.bias", {lat2}, &t.bq));
    return 0;
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

size_t dt_size(int dt) { return dt == DT_F32 ? 4 : 2; }

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
    float* s32[2] = {cx.f(maxe), cx.f(maxe)};
    half_t* s16[2] = {cx.h(2 * maxe), cx.h(2 * maxe)};
    int cur = 0;
    auto next = [&](bool need16, int C) {
        cur ^= 1;
        TV v; v.p = s32[cur]; v.dt = DT_F32; v.m16 = need16 ? s16[cur] : nullptr; v.lo_off = need16 ? C : 0;
        return v;
    };
    const int C0 = c.block_out_channels[0];
    const char* px = (const char*)a.px + (size_t)n * 3 * H * W * dt_size(a.pdt);
    RUN(cx, op_vae_conv_in(px, a.pdt, t.conv_in.w, t.conv_in.b, s32[0], H, W, C0, cx.s));
    TV x; x.p = s32[0]; x.dt = DT_F32;
    cur = 0;
    int h = H, w = W;
    for (int i = 0; i < nl; ++i) {
        const VaeLevel& lv = t.levels[i];
        for (int j = 0; j < (int)lv.res.size(); ++j) {
            // the fp16 mirror is needed where the next op reads the stream as a convolution operand: the downsample, or a shortcut
            bool need16 = false;
            if (j + 1 < (int)lv.res.size()) need16 = lv.res[j + 1].has_shortcut;
            else if (lv.down) need16 = true;
            TV y = next(need16, lv.res[j].Cout);
            TRY(run_resnet(cx, lv.res[j], x, y, 1, h, w, 1, nullptr, 0, eps));
            x = y;
        }
        if (lv.down) {
            TV y = next(t.levels[i + 1].res[0].has_shortcut, lv.res.back().Cout);
            ConvOpts o; o.stride = 2; o.tap_origin = 1;
            TRY(run_conv(cx, lv.down_conv, x.m16, y, 1, h, w, o));      // the split mirror, as a split operand
            h /= 2; w /= 2;
            x = y;
        }
    }
    const int L = h * w;
    const int Ct = c.block_out_channels[nl - 1];
    { TV y = next(false, Ct); TRY(run_resnet(cx, t.mid0, x, y, 1, h, w, 1, nullptr, 0, eps)); x = y; }
    { TV y = next(false, Ct); TRY(run_vae_mid_attention(cx, t.attn_gn, t.qkv, t.attn_out, Ct, eps, x, y, L)); x = y; }
    { TV y = next(false, Ct); TRY(run_resnet(cx, t.mid1, x, y, 1, h, w, 1, nullptr, 0, eps)); x = y; }
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
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    t.ar.off = 0; t.ar.peak = 0;
    Ctx dry{&t.ar, s, true};
    dry.f32stream = true;
    TRY(run_image(dry, t, a, 0));
    const size_t need = workspace_bytes(dry);
    CTRL_CHECK(!capturing || need <= t.ar.cap, "vae encoder: the first forward of a larger image allocates its workspace and cannot run "
                                               "under stream capture -- run it eagerly once, then capture");
    TRY(t.ar.ensure(need));
    Ctx cx{&t.ar, s, false};
    cx.f32stream = true;
    cx.capturing = capturing;
    cx.stats_total = dry.stats_total;
    for (int n = 0; n < N; ++n) {
        t.ar.off = 0;
        TRY(run_image(cx, t, a, n));
    }
    return t.leave(s, capturing);
}

}  // namespace

#define S(stream) ((hipStream_t)(stream))

extern "C" {

int ctrl_vae_encoder_param_count(const ctrl_vae_encoder_config* cfg) {
    if (!cfg || validate(*cfg)) return -1;
    SpecCollector sc; VaeEncoder t;
    t.cfg = *cfg;
    if (build_vae(sc, t)) return -1;
    return (int)sc.entries.size();
}

int ctrl_vae_encoder_param_spec(const ctrl_vae_encoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "vae_encoder_param_spec: null argument");
    TRY(validate(*cfg));
    SpecCollector sc; VaeEncoder t;
    t.cfg = *cfg;
    TRY(build_vae(sc, t));
    CTRL_CHECK(i >= 0 && i < (int)sc.entries.size(), "vae_encoder_param_spec: index out of range");
    std::strncpy(name, sc.entries[i].name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
    *ndim = (int)sc.entries[i].shape.size();
    for (int k = 0; k < 6; ++k) shape[k] = k < *ndim ? sc.entries[i].shape[k] : 1;
    return 0;
}

int ctrl_vae_encoder_create(const ctrl_vae_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                            ctrl_vae_encoder** out) {
    CTRL_CHECK(cfg && out && (tensors || n_tensors == 0), "vae_encoder_create: null argument");
    *out = nullptr;
    TRY(validate(*cfg));
    VaeEncoder* t = new VaeEncoder();
    t->cfg = *cfg;
    int rc = t->init_base(n_tensors ? tensors[0].data : nullptr);
    DeviceGuard dg(t->device);
    if (!rc) {
        t->pk = new Packer(tensors, n_tensors, (hipStream_t)stream);
        rc = build_vae(*t->pk, *t);
        if (!rc) rc = pad_conv_out(*t, (hipStream_t)stream);
        if (!rc) rc = t->pk->finish();
    }
    if (rc) { delete t; return rc; }
    *out = (ctrl_vae_encoder*)t;
    return 0;
}

void ctrl_vae_encoder_destroy(ctrl_vae_encoder* h) {
    if (!h) return;
    VaeEncoder* t = (VaeEncoder*)h;
    DeviceGuard dg(t->device);
    (void)hipDeviceSynchronize();        // queued launches and captured graphs may still address the workspace
    delete t;
}

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
