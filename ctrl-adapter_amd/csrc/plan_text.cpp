// CLIP text encoder plan (transformers CLIPTextModel, the text_encoder that ControlNetHelper.encode_controlnet_prompt runs,
// model/ctrl_helper.py:300-457): weights packed once, a forward of 2 + 7 * layers launches (85 for SD-1.5's twelve layers):
//   embed + LN1(0) | per layer: Q|K|V GEMM, causal attention, out_proj (+ residual), LN2, fc1 (quick_gelu epilogue), fc2 (+ residual),
//   LN1(next) | final LayerNorm + pooled row.
// Residual stream fp32 (two ping-pong buffers), GEMM operands fp16.  Every GEMM runs in the one pinned form (op_igemm_pinned) and every
// other kernel computes rows or (prompt, head) pairs on their own, so a prompt's outputs are bit-identical whatever the batch it is in.
// The ext plan (ctrl_text_encoder_create_ext: SDXL's OpenCLIP bigG text_encoder_2) adds exact gelu, hidden sizes up to 2048, the
// fp32 text projection of the pooled row and the few-row GEMM of text_gemm.hip (gemm_form 1), equally batch-invariant.
#include "plan_clip.h"
#include <cmath>

namespace {

struct TextEncoder : StandalonePlan {
    ctrl_text_encoder_config cfg{};
    ctrl_text_encoder_ext ext{};     // zeros: quick_gelu, no projection, the pinned GEMM (what ctrl_text_encoder_create builds)
    float* proj = nullptr;           // text_projection.weight fp32 [projection_dim][hidden]
    float* tok = nullptr;
    float* pos = nullptr;
    std::vector<ClipLayer> layers;
    Norm final_ln;
    int* bad = nullptr;          // device flag word: an id outside the vocabulary was clamped
    ~TextEncoder() {
        if (bad) (void)hipFree(bad);
    }
};

int validate(const ctrl_text_encoder_config& c, int max_hidden) {
    CTRL_CHECK(c.vocab_size >= 1 && c.num_hidden_layers >= 1, "text encoder: vocab_size and num_hidden_layers must be positive");
    CTRL_CHECK(c.hidden_size >= 64 && c.hidden_size <= max_hidden && c.hidden_size % 64 == 0,
               max_hidden == 1024 ? "text encoder: hidden_size must be a multiple of 64 up to 1024"
                                  : "text encoder: hidden_size must be a multiple of 64 up to 2048");
    CTRL_CHECK(c.num_attention_heads >= 1 && c.hidden_size == 64 * c.num_attention_heads, "text encoder: head_dim must be 64");
    CTRL_CHECK(c.intermediate_size >= 64 && c.intermediate_size % 64 == 0, "text encoder: intermediate_size must be a multiple of 64");
    CTRL_CHECK(c.max_position_embeddings >= 1 && c.max_position_embeddings <= 128, "text encoder: max_position_embeddings must be <= 128");
    CTRL_CHECK(c.layer_norm_eps > 0.f, "text encoder: layer_norm_eps must be positive");
    return 0;
}

int build_text(ParamSink& ps, TextEncoder& t) {
    const ctrl_text_encoder_config& c = t.cfg;
    const int C = c.hidden_size;
    TRY(ps.raw_f32("text_model.embeddings.token_embedding.weight", {c.vocab_size, C}, &t.tok));
    TRY(ps.raw_f32("text_model.embeddings.position_embedding.weight", {c.max_position_embeddings, C}, &t.pos));
    TRY(build_clip_layers(ps, "text_model.encoder.layers.", c.num_hidden_layers, C, c.intermediate_size, &t.layers));
    TRY(ps.norm("text_model.final_layer_norm", C, &t.final_ln));
    if (t.ext.projection_dim > 0) TRY(ps.raw_f32("text_projection.weight", {t.ext.projection_dim, C}, &t.proj));
    return 0;
}

int validate_ext(const ctrl_text_encoder_ext& e) {
    CTRL_CHECK(e.hidden_act == 0 || e.hidden_act == 1, "text encoder: hidden_act must be 0 (quick_gelu) or 1 (gelu)");
    CTRL_CHECK(e.projection_dim >= 0 && e.projection_dim <= 65536, "text encoder: projection_dim must be 0 .. 65536");
    CTRL_CHECK(e.gemm_form == 0 || e.gemm_form == 1, "text encoder: gemm_form must be 0 (pinned) or 1 (few-row GEMM)");
    CTRL_CHECK(e.reserved == 0, "text encoder: ctrl_text_encoder_ext.reserved must be 0");
    return 0;
}

// hidden_index -1: every state into hidden [layers + 1][N][L][C]; k >= 0: state k alone into hidden [N][L][C], and with no
// last / pooled / embeds requested the layers after k are not run
int forward(TextEncoder& t, const int64_t* ids, int N, int L, void* last, void* pooled, void* embeds, void* hidden, int hidden_index, int odt,
            hipStream_t s) {
    const ctrl_text_encoder_config& c = t.cfg;
    CTRL_CHECK(ids != nullptr && (last || pooled || embeds || hidden), "text encoder: ids and at least one output are required");
    CTRL_CHECK(N >= 1 && L >= 1 && L <= c.max_position_embeddings, "text encoder: need N >= 1 and 1 <= L <= max_position_embeddings");
    CTRL_CHECK(odt == DT_F32 || odt == DT_F16 || odt == DT_BF16, "text encoder: out_dtype must be fp32, fp16 or bf16");
    CTRL_CHECK((long)N * L <= (1L << 24), "text encoder: batch too large");
    CTRL_CHECK(hidden_index >= -1 && hidden_index <= c.num_hidden_layers, "text encoder: hidden_index must be -1 .. num_hidden_layers");
    CTRL_CHECK(!embeds || t.proj, "text encoder: text_embeds needs a plan with a text projection (projection_dim > 0)");
    const int C = c.hidden_size, I = c.intermediate_size, M = N * L;
    const float eps = c.layer_norm_eps;
    const int layers = clip_layers_to_run(last || pooled || embeds, hidden_index, c.num_hidden_layers);
    // workspace: two fp32 stream buffers, the fp16 LayerNorm output, Q | K | V, the attention output, the MLP hidden activation
    // (+ the linears' scratch and the fp32 pooled rows of the projection)
    const size_t b_x = al256((size_t)M * C * 4), b_h = al256((size_t)M * C * 2), b_qkv = al256((size_t)M * 3 * C * 2),
                 b_ff = al256((size_t)M * I * 2), b_lin = al256(lin_scratch_bytes(t.ext.gemm_form, t.ext.hidden_act, M, C, I)),
                 b_p32 = t.proj ? al256((size_t)N * C * 4) : 0;
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    TRY(t.reserve(2 * b_x + 2 * b_h + b_qkv + b_ff + b_lin + b_p32, capturing, "text encoder", "batch"));
    char* p = t.ar.base;
    ClipBufs b;
    b.xa = (float*)p; p += b_x;
    b.xb = (float*)p; p += b_x;
    b.h16 = (half_t*)p; p += b_h;
    b.ao = (half_t*)p; p += b_h;
    b.qkv = (half_t*)p; p += b_qkv;
    b.ff = (half_t*)p; p += b_ff;
    b.lws.p = b_lin ? (float*)p : nullptr; b.lws.bytes = b_lin; p += b_lin;
    float* p32 = b_p32 ? (float*)p : nullptr;
    const ClipSnapshot snap{hidden, hidden_index, odt, (size_t)M * C};
    TRY(op_text_embed(ids, t.tok, t.pos, c.vocab_size, N, L, C, b.xa, t.layers[0].ln1.g, t.layers[0].ln1.b, eps, b.h16, t.bad, s));
    TRY(snap(0, b.xa, s));
    const float scale = 1.0f / std::sqrt(64.0f);
    TRY(run_clip_layers(t.layers, layers, t.ext.gemm_form, t.ext.hidden_act, M, C, eps, b, snap, s,
                        [&] { return op_text_attn(b.qkv, 3L * C, b.ao, C, N, L, c.num_attention_heads, scale, s); }));
    if (last || pooled || embeds)
        TRY(op_text_final_ext(b.xa, DT_F32, M, C, t.final_ln.g, t.final_ln.b, eps, last, odt, ids, L, c.eos_token_id, pooled,
                              embeds ? p32 : nullptr, s));
    if (embeds) TRY(op_text_proj(p32, t.proj, N, C, t.ext.projection_dim, embeds, odt, s));
    return t.leave(s, capturing);
}

// the device flag word of the ids, after the build
int alloc_bad(TextEncoder& t, hipStream_t) {
    if (hipMalloc((void**)&t.bad, sizeof(int)) != hipSuccess) { ctrl_set_error("text_encoder_create: hipMalloc failed"); return 1; }
    if (hipMemset(t.bad, 0, sizeof(int)) != hipSuccess) { ctrl_set_error("text_encoder_create: hipMemset failed"); return 1; }
    return 0;
}

}  // namespace

extern "C" {

int ctrl_text_encoder_create(const ctrl_text_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                             ctrl_text_encoder** out) {
    return plan_create<TextEncoder>("text_encoder_create", cfg, tensors, n_tensors, stream, (void**)out,
                                    [](const ctrl_text_encoder_config& c) { return validate(c, 1024); }, build_text, alloc_bad);
}

int ctrl_text_encoder_create_ext(const ctrl_text_encoder_config* cfg, const ctrl_text_encoder_ext* ext, const ctrl_tensor_ref* tensors,
                                 int n_tensors, void* stream, ctrl_text_encoder** out) {
    CTRL_CHECK(ext, "text_encoder_create_ext: null argument");
    return plan_create<TextEncoder>("text_encoder_create_ext", cfg, tensors, n_tensors, stream, (void**)out,
                                    [&](const ctrl_text_encoder_config& c) { TRY(validate(c, 2048)); return validate_ext(*ext); },
                                    [&](ParamSink& ps, TextEncoder& t) { t.ext = *ext; return build_text(ps, t); }, alloc_bad);
}

void ctrl_text_encoder_destroy(ctrl_text_encoder* h) { plan_destroy<TextEncoder>(h); }

int ctrl_text_encoder_forward(ctrl_text_encoder* h, const int64_t* input_ids, int N, int L, void* last_hidden, void* pooled,
                              void* hidden_states, int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "text_encoder_forward: null plan");
    TextEncoder* t = (TextEncoder*)h;
    DeviceGuard dg(t->device);
    return forward(*t, input_ids, N, L, last_hidden, pooled, nullptr, hidden_states, -1, out_dtype, S(stream));
}

int ctrl_text_encoder_forward_ext(ctrl_text_encoder* h, const int64_t* input_ids, int N, int L, void* last_hidden, void* pooled,
                                  void* text_embeds, void* hidden_states, int hidden_index, int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "text_encoder_forward_ext: null plan");
    TextEncoder* t = (TextEncoder*)h;
    DeviceGuard dg(t->device);
    return forward(*t, input_ids, N, L, last_hidden, pooled, text_embeds, hidden_states, hidden_index, out_dtype, S(stream));
}

int ctrl_text_encoder_id_status(ctrl_text_encoder* h, int reset) {
    if (!h) return -1;
    TextEncoder* t = (TextEncoder*)h;
    DeviceGuard dg(t->device);
    int v = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, t->bad, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (reset && v && hipMemset(t->bad, 0, sizeof(int)) != hipSuccess) return -1;
    return v;
}

int ctrl_op_text_embed(const int64_t* ids, const float* tok, const float* pos, int V, int N, int L, int C, float* x,
                       const float* gamma, const float* beta, float eps, void* y, int32_t* bad, void* stream) {
    return op_text_embed(ids, tok, pos, V, N, L, C, x, gamma, beta, eps, (half_t*)y, bad, S(stream));
}

int ctrl_op_text_attn(const void* qkv, int64_t ld, void* out, int64_t ldo, int N, int L, int heads, float scale, void* stream) {
    return op_text_attn((const half_t*)qkv, (long)ld, (half_t*)out, (long)ldo, N, L, heads, scale, S(stream));
}

int ctrl_op_text_final_ln(const void* x, int x_dtype, int rows, int C, const float* gamma, const float* beta, float eps,
                          void* y, int y_dtype, const int64_t* ids, int L, int eos_token_id, void* pooled, void* stream) {
    return op_text_final(x, x_dtype, rows, C, gamma, beta, eps, y, y_dtype, ids, L, eos_token_id, pooled, S(stream));
}

int64_t ctrl_text_gemm_ws_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    return (int64_t)text_gemm_ws_bytes(M, N, K);
}

int ctrl_op_text_gemm(const void* x, const void* W, const float* bias, int M, int N, int K, int act, const float* res, void* y, int y_dtype,
                      void* ws, int64_t ws_bytes, void* stream) {
    CTRL_CHECK(ws_bytes >= 0, "text_gemm: ws_bytes must be >= 0");
    return op_text_gemm((const half_t*)x, (const half_t*)W, bias, M, N, K, act, res, y, y_dtype, (float*)ws, (size_t)ws_bytes, S(stream));
}

int ctrl_op_text_gemm_finish(const float* ws, int splits, int M, int N, const float* bias, int act, const float* res, int64_t ldres, void* y,
                             int y_dtype, int64_t ldy, void* stream) {
    return op_text_gemm_finish(ws, splits, M, N, bias, act, res, (long)ldres, y, y_dtype, (long)ldy, S(stream));
}

int ctrl_op_text_proj(const float* pooled32, const float* Wp, int N, int C, int P, void* out, int out_dtype, void* stream) {
    return op_text_proj(pooled32, Wp, N, C, P, out, out_dtype, S(stream));
}

int ctrl_op_text_store(const float* x, void* y, int y_dtype, int64_t n, void* stream) {
    CTRL_CHECK(n >= 0, "text_store: n must be >= 0");
    return op_text_store(x, y, y_dtype, (size_t)n, S(stream));
}

int ctrl_op_text_final_ln_ext(const void* x, int x_dtype, int rows, int C, const float* gamma, const float* beta, float eps,
                              void* y, int y_dtype, const int64_t* ids, int L, int eos_token_id, void* pooled, float* pooled32, void* stream) {
    return op_text_final_ext(x, x_dtype, rows, C, gamma, beta, eps, y, y_dtype, ids, L, eos_token_id, pooled, pooled32, S(stream));
}

}  // extern "C"
