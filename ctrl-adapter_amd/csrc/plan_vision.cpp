// CLIP vision tower plan (transformers CLIPVisionModelWithProjection, the image_encoder of SVD and I2VGen-XL: CLIP ViT-H/14; the
// pipelines' _encode_image, svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212, i2vgen_xl/...:366-396): weights packed once,
// a forward of 3 + 9 * layers + 2 launches with exact gelu on the pinned form (its separate fp32 gelu pass; 8 per layer otherwise):
//   patchify (+ normalise) | patch GEMM | embed + pre_layrnorm + LN1(0) | per layer: Q|K|V GEMM, V^T, flash attention, out_proj
//   (+ residual), LN2, fc1 (+ act), fc2 (+ residual), LN1(next) | last hidden state | post_layernorm of the class rows | projection.
// The text plan's loop (plan_text.cpp) with the non-causal flash attention of the adapter path in place of the causal text kernel.
// Q | K | V leave the GEMM row-major and vision_vt_kernel writes V^T with zeroed pad columns: the pinned GEMM's transposed epilogue
// needs L % 8 == 0 and ViT-H/14 has L = 257.  Residual stream fp32, GEMM operands fp16.  Every GEMM runs in one batch-invariant form
// (gemm_form 0: the pinned 64 x 64 x 64 implicit GEMM; 1: the few-row split-K GEMM of text_gemm.hip; the patch GEMM is always the
// pinned one) and every other kernel computes rows, tiles of one image or (image, head, query tile) on its own: an image's outputs are
// bit-identical whatever the batch it is in.
#include "plan_clip.h"
#include <cmath>

namespace {

struct VisionEncoder : StandalonePlan {
    ctrl_vision_encoder_config cfg{};
    int P = 0, L = 0, K = 0, Kpad = 0, Lkpad = 0, D = 0;
    float* cls = nullptr;          // class_embedding fp32 [C]
    float* pos = nullptr;          // position_embedding fp32 [L][C]
    float* patch32 = nullptr;      // patch_embedding.weight fp32 [C][3][p][p] (packed to patch_w)
    half_t* patch_w = nullptr;     // fp16 [C][Kpad]
    float* proj = nullptr;         // visual_projection.weight fp32 [P][C]
    Norm pre_ln, post_ln;
    std::vector<ClipLayer> layers;
};

int validate(const ctrl_vision_encoder_config& c) {
    CTRL_CHECK(c.hidden_size >= 64 && c.hidden_size <= 2048 && c.hidden_size % 64 == 0,
               "vision encoder: hidden_size must be a multiple of 64 up to 2048");
    CTRL_CHECK(c.num_attention_heads >= 1 && c.hidden_size % c.num_attention_heads == 0, "vision encoder: heads must divide hidden_size");
    const int D = c.hidden_size / c.num_attention_heads;
    CTRL_CHECK(D == 40 || D == 64 || D == 80 || D == 160, "vision encoder: head_dim must be 40, 64, 80 or 160");
    CTRL_CHECK(c.intermediate_size >= 64 && c.intermediate_size % 64 == 0, "vision encoder: intermediate_size must be a multiple of 64");
    CTRL_CHECK(c.num_hidden_layers >= 1, "vision encoder: num_hidden_layers must be positive");
    CTRL_CHECK(c.patch_size >= 1 && c.image_size >= c.patch_size && c.image_size % c.patch_size == 0,
               "vision encoder: image_size must be a positive multiple of patch_size");
    const long G = c.image_size / c.patch_size;
    CTRL_CHECK(G * G + 1 <= 577, "vision encoder: at most 577 tokens ((image_size / patch_size)^2 + 1)");
    CTRL_CHECK(c.projection_dim >= 1 && c.projection_dim <= 65536, "vision encoder: projection_dim must be 1 .. 65536");
    CTRL_CHECK(c.hidden_act == 0 || c.hidden_act == 1, "vision encoder: hidden_act must be 0 (quick_gelu) or 1 (gelu)");
    CTRL_CHECK(c.gemm_form == 0 || c.gemm_form == 1, "vision encoder: gemm_form must be 0 (pinned) or 1 (few-row GEMM)");
    CTRL_CHECK(c.layer_norm_eps > 0.f, "vision encoder: layer_norm_eps must be positive");
    return 0;
}

// the token / patch geometry of the config, then the parameters
int build_vision(ParamSink& ps, VisionEncoder& t) {
    const ctrl_vision_encoder_config& c = t.cfg;
    const int C = c.hidden_size, p = c.patch_size, G = c.image_size / p;
    t.P = G * G;
    t.L = t.P + 1;
    t.K = 3 * p * p;
    t.Kpad = (t.K + 63) / 64 * 64;
    t.Lkpad = (t.L + 63) / 64 * 64;
    t.D = C / c.num_attention_heads;
    TRY(ps.raw_f32("vision_model.embeddings.class_embedding", {C}, &t.cls));
    TRY(ps.raw_f32("vision_model.embeddings.patch_embedding.weight", {C, 3, p, p}, &t.patch32));
    TRY(ps.raw_f32("vision_model.embeddings.position_embedding.weight", {t.L, C}, &t.pos));
    TRY(ps.norm("vision_model.pre_layrnorm", C, &t.pre_ln));
    TRY(build_clip_layers(ps, "vision_model.encoder.layers.", c.num_hidden_layers, C, c.intermediate_size, &t.layers));
    TRY(ps.norm("vision_model.post_layernorm", C, &t.post_ln));
    TRY(ps.raw_f32("visual_projection.weight", {c.projection_dim, C}, &t.proj));
    return 0;
}

// patch_embedding.weight as the patch GEMM's fp16 [C][Kpad] operand
int pack_patch_w(VisionEncoder& t, hipStream_t s) {
    TRY(t.pk->dalloc((size_t)t.cfg.hidden_size * t.Kpad * sizeof(half_t), (void**)&t.patch_w));
    return op_vision_pack_patch(t.patch32, t.cfg.hidden_size, t.K, t.Kpad, t.patch_w, s);
}

int collect(const ctrl_vision_encoder_config& c, SpecCollector& sc) {
    TRY(validate(c));
    VisionEncoder t;
    t.cfg = c;
    return build_vision(sc, t);
}

int forward(VisionEncoder& t, const void* px, int pdt, int N, const float* mean_std, void* last, void* pooled, void* embeds, void* hidden,
            int hidden_index, int odt, hipStream_t s) {
    const ctrl_vision_encoder_config& c = t.cfg;
    CTRL_CHECK(px != nullptr && (last || pooled || embeds || hidden), "vision encoder: pixels and at least one output are required");
    CTRL_CHECK(pdt == DT_F32 || pdt == DT_F16 || pdt == DT_BF16 || pdt == CTRL_U8_NHWC,
               "vision encoder: pixel dtype must be fp32, fp16, bf16 (NCHW) or uint8 (NHWC)");
    CTRL_CHECK(N >= 1 && (long)N * t.L <= (1L << 22), "vision encoder: need 1 <= N and N * tokens <= 2^22");
    CTRL_CHECK(odt == DT_F32 || odt == DT_F16 || odt == DT_BF16, "vision encoder: out_dtype must be fp32, fp16 or bf16");
    CTRL_CHECK(hidden_index >= -1 && hidden_index <= c.num_hidden_layers, "vision encoder: hidden_index must be -1 .. num_hidden_layers");
    const int C = c.hidden_size, I = c.intermediate_size, L = t.L, M = N * L, Mp = N * t.P;
    const float eps = c.layer_norm_eps;
    const int layers = clip_layers_to_run(last || pooled || embeds, hidden_index, c.num_hidden_layers);
    // workspace: im2col rows + the patch GEMM output, two fp32 stream buffers, the fp16 LayerNorm output, the attention output,
    // Q | K | V rows, V^T, the MLP hidden activation, the linears' scratch and the fp32 pooled rows
    const size_t b_pa = al256((size_t)Mp * t.Kpad * 2), b_po = al256((size_t)Mp * C * 4), b_x = al256((size_t)M * C * 4),
                 b_h = al256((size_t)M * C * 2), b_qkv = al256((size_t)M * 3 * C * 2), b_vt = al256((size_t)N * C * t.Lkpad * 2),
                 b_ff = al256((size_t)M * I * 2), b_lin = al256(lin_scratch_bytes(c.gemm_form, c.hidden_act, M, C, I)),
                 b_p32 = al256((size_t)N * C * 4);
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    TRY(t.reserve(b_pa + b_po + 2 * b_x + 2 * b_h + b_qkv + b_vt + b_ff + b_lin + b_p32, capturing, "vision encoder", "batch"));
    char* p = t.ar.base;
    ClipBufs b;
    half_t* pa = (half_t*)p; p += b_pa;
    float* po = (float*)p; p += b_po;
    b.xa = (float*)p; p += b_x;
    b.xb = (float*)p; p += b_x;
    b.h16 = (half_t*)p; p += b_h;
    b.ao = (half_t*)p; p += b_h;
    b.qkv = (half_t*)p; p += b_qkv;
    half_t* vt = (half_t*)p; p += b_vt;
    b.ff = (half_t*)p; p += b_ff;
    b.lws.p = b_lin ? (float*)p : nullptr; b.lws.bytes = b_lin; p += b_lin;
    float* p32 = (float*)p;
    const float* xa = b.xa;
    const ClipSnapshot snap{hidden, hidden_index, odt, (size_t)M * C};     // state 0: after pre_layrnorm
    TRY(op_vision_patchify(px, pdt, N, c.image_size, c.patch_size, mean_std, pa, t.Kpad, s));
    TRY(pinned_linear(pa, t.patch_w, nullptr, C, t.Kpad, po, DT_F32, Mp, nullptr, 0, s));
    TRY(op_vision_embed(po, t.cls, t.pos, N, L, C, t.pre_ln.g, t.pre_ln.b, t.layers[0].ln1.g, t.layers[0].ln1.b, eps, b.xa, b.h16, s));
    TRY(snap(0, xa, s));
    AttnArgs at = {};
    at.Q = b.qkv; at.ldq = 3 * C; at.K = b.qkv + C; at.ldk = 3 * C; at.Vt = vt; at.Lkpad = t.Lkpad; at.kvB = N;
    at.O = b.ao; at.ldo = C; at.B = N; at.heads = c.num_attention_heads; at.D = t.D; at.Lq = L; at.Lk = L;
    at.scale = 1.0f / std::sqrt((float)t.D);
    TRY(run_clip_layers(t.layers, layers, c.gemm_form, c.hidden_act, M, C, eps, b, snap, s, [&] {
        TRY(op_vision_vt(b.qkv + 2 * C, 3L * C, vt, N, L, C, t.Lkpad, s));
        return op_flash_attn(at, s);
    }));
    if (last) TRY(op_text_store(xa, last, odt, (size_t)M * C, s));
    if (pooled || embeds) TRY(op_vision_cls_ln(xa, N, L, C, t.post_ln.g, t.post_ln.b, eps, pooled, odt, p32, s));
    if (embeds) TRY(op_text_proj(p32, t.proj, N, C, c.projection_dim, embeds, odt, s));
    return t.leave(s, capturing);
}

}  // namespace

extern "C" {

int ctrl_vision_encoder_param_count(const ctrl_vision_encoder_config* cfg) {
    SpecCollector sc;
    return (cfg && !collect(*cfg, sc)) ? (int)sc.entries.size() : -1;
}

int ctrl_vision_encoder_param_spec(const ctrl_vision_encoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(cfg && name && shape && ndim && name_len >= 1, "vision_encoder_param_spec: null argument");
    SpecCollector sc;
    TRY(collect(*cfg, sc));
    return spec_entry(sc, i, "vision_encoder_param_spec", name, name_len, shape, ndim);
}

int ctrl_vision_encoder_create(const ctrl_vision_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                               ctrl_vision_encoder** out) {
    return plan_create<VisionEncoder>("vision_encoder_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_vision,
                                      pack_patch_w);
}

void ctrl_vision_encoder_destroy(ctrl_vision_encoder* h) { plan_destroy<VisionEncoder>(h); }

int ctrl_vision_encoder_forward(ctrl_vision_encoder* h, const void* pixels, int pixel_dtype, int N, const float* mean_std,
                                void* last_hidden, void* pooled, void* image_embeds, void* hidden_states, int hidden_index,
                                int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "vision_encoder_forward: null plan");
    VisionEncoder* t = (VisionEncoder*)h;
    DeviceGuard dg(t->device);
    return forward(*t, pixels, pixel_dtype, N, mean_std, last_hidden, pooled, image_embeds, hidden_states, hidden_index, out_dtype, S(stream));
}

int ctrl_op_vision_patchify(const void* pixels, int pixel_dtype, int N, int image_size, int patch_size, const float* mean_std, void* out,
                            int Kpad, void* stream) {
    return op_vision_patchify(pixels, pixel_dtype, N, image_size, patch_size, mean_std, (half_t*)out, Kpad, S(stream));
}

int ctrl_op_vision_embed(const float* patch_out, const float* class_embedding, const float* pos, int N, int L, int C, const float* pre_g,
                         const float* pre_b, const float* ln1_g, const float* ln1_b, float eps, float* x, void* y, void* stream) {
    return op_vision_embed(patch_out, class_embedding, pos, N, L, C, pre_g, pre_b, ln1_g, ln1_b, eps, x, (half_t*)y, S(stream));
}

int ctrl_op_vision_cls_ln(const float* x, int N, int L, int C, const float* gamma, const float* beta, float eps, void* pooled,
                          int out_dtype, float* pooled32, void* stream) {
    return op_vision_cls_ln(x, N, L, C, gamma, beta, eps, pooled, out_dtype, pooled32, S(stream));
}

int ctrl_op_clip_resize_aa(const void* src, int src_dtype, int N, int H, int W, int OH, int OW, const float* mean_std, void* out,
                           int out_dtype, void* stream) {
    return op_clip_resize_aa(src, src_dtype, N, H, W, OH, OW, mean_std, out, out_dtype, S(stream));
}

int ctrl_op_vision_vt(const void* v, int64_t ld, void* vt, int N, int L, int C, int Lkpad, void* stream) {
    return op_vision_vt((const half_t*)v, (long)ld, (half_t*)vt, N, L, C, Lkpad, S(stream));
}

}  // extern "C"
