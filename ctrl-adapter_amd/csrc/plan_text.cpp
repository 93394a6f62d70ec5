// CLIP text encoder plan (transformers CLIPTextModel, the text_encoder that ControlNetHelper.encode_controlnet_prompt runs,
// model/ctrl_helper.py:300-457): weights packed once, a forward of 2 + 7 * layers launches (85 for SD-1.5's twelve layers):
//   embed + LN1(0) | per layer: Q|K|V GEMM, causal attention, out_proj (+ residual), LN2, fc1 (quick_gelu epilogue), fc2 (+ residual),
//   LN1(next) | final LayerNorm + pooled row.
// Residual stream fp32 (two ping-pong buffers), GEMM operands fp16.  Every GEMM runs in the one pinned form (op_igemm_pinned) and every
// other kernel computes rows or (prompt, head) pairs on their own, so a prompt's outputs are bit-identical whatever the batch it is in.
#include "plan_common.h"
#include <cmath>

namespace {

struct TextLayer {
    Norm ln1, ln2;
    Lin qkv, out, fc1, fc2;
};

struct TextEncoder : PlanBase {
    ctrl_text_encoder_config cfg{};
    Packer* pk = nullptr;
    float* tok = nullptr;
    float* pos = nullptr;
    std::vector<TextLayer> layers;
    Norm final_ln;
    Arena ar;
    int* bad = nullptr;          // device flag word: an id outside the vocabulary was clamped
    ~TextEncoder() {
        if (pk) { pk->release_all(); delete pk; }
        if (bad) (void)hipFree(bad);
    }
};

int validate(const ctrl_text_encoder_config& c) {
    CTRL_CHECK(c.vocab_size >= 1 && c.num_hidden_layers >= 1, "text encoder: vocab_size and num_hidden_layers must be positive");
    CTRL_CHECK(c.hidden_size >= 64 && c.hidden_size <= 1024 && c.hidden_size % 64 == 0,
               "text encoder: hidden_size must be a multiple of 64 up to 1024");
    CTRL_CHECK(c.num_attention_heads >= 1 && c.hidden_size == 64 * c.num_attention_heads, "text encoder: head_dim must be 64");
    CTRL_CHECK(c.intermediate_size >= 64 && c.intermediate_size % 64 == 0, "text encoder: intermediate_size must be a multiple of 64");
    CTRL_CHECK(c.max_position_embeddings >= 1 && c.max_position_embeddings <= 128, "text encoder: max_position_embeddings must be <= 128");
    CTRL_CHECK(c.layer_norm_eps > 0.f, "text encoder: layer_norm_eps must be positive");
    return 0;
}

int build_text(ParamSink& ps, TextEncoder& t) {
    const ctrl_text_encoder_config& c = t.cfg;
    const int C = c.hidden_size, I = c.intermediate_size;
    TRY(ps.raw_f32("text_model.embeddings.token_embedding.weight", {c.vocab_size, C}, &t.tok));
    TRY(ps.raw_f32("text_model.embeddings.position_embedding.weight", {c.max_position_embeddings, C}, &t.pos));
    t.layers.resize(c.num_hidden_layers);
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        const std::string pre = "text_model.encoder.layers." + std::to_string(i) + ".";
        TextLayer& l = t.layers[i];
        TRY(ps.norm(pre + "layer_norm1", C, &l.ln1));
        TRY(ps.linear_cat({pre + "self_attn.q_proj", pre + "self_attn.k_proj", pre + "self_attn.v_proj"}, {C, C, C}, C, true, &l.qkv));
        TRY(ps.linear(pre + "self_attn.out_proj", C, C, true, false, &l.out));
        TRY(ps.norm(pre + "layer_norm2", C, &l.ln2));
        TRY(ps.linear(pre + "mlp.fc1", I, C, true, false, &l.fc1));
        TRY(ps.linear(pre + "mlp.fc2", C, I, true, false, &l.fc2));
    }
    TRY(ps.norm("text_model.final_layer_norm", C, &t.final_ln));
    return 0;
}

// row-major linear on the pinned GEMM: y[M][N] (dtype of y) = act(x[M][K] W^T + b) (+ fp32 residual)
int linear(const Lin& l, const half_t* x, void* y, int y_dt, int M, const float* res, int act, hipStream_t s) {
    IGemmArgs g = {};
    g.A = x; g.lda = l.K; g.mode = IG_ROWS; g.Cin = l.K; g.taps = 1;
    g.W = l.w; g.M = M; g.Nout = l.N; g.Ktot = l.K; g.bias = l.b; g.scale = 1.f; g.act = act;
    g.res = res; g.ldres = l.N; g.res_f32 = res ? 1 : 0;
    g.nseg = 1;
    g.seg[0] = IGemmSeg{y, l.N, 0, l.N, SEG_ROW, y_dt, 1, 0, nullptr};
    return op_igemm_pinned(g, s);
}

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

int forward(TextEncoder& t, const int64_t* ids, int N, int L, void* last, void* pooled, void* hidden, int odt, hipStream_t s) {
    const ctrl_text_encoder_config& c = t.cfg;
    CTRL_CHECK(ids != nullptr && (last || pooled || hidden), "text encoder: ids and at least one output are required");
    CTRL_CHECK(N >= 1 && L >= 1 && L <= c.max_position_embeddings, "text encoder: need N >= 1 and 1 <= L <= max_position_embeddings");
    CTRL_CHECK(odt == DT_F32 || odt == DT_F16 || odt == DT_BF16, "text encoder: out_dtype must be fp32, fp16 or bf16");
    CTRL_CHECK((long)N * L <= (1L << 24), "text encoder: batch too large");
    const int C = c.hidden_size, I = c.intermediate_size, M = N * L;
    const float eps = c.layer_norm_eps;
    // workspace: two fp32 stream buffers, the fp16 LayerNorm output, Q | K | V, the attention output, the MLP hidden activation
    const size_t b_x = al256((size_t)M * C * 4), b_h = al256((size_t)M * C * 2), b_qkv = al256((size_t)M * 3 * C * 2),
                 b_ff = al256((size_t)M * I * 2);
    const size_t need = 2 * b_x + 2 * b_h + b_qkv + b_ff;
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    CTRL_CHECK(!capturing || need <= t.ar.cap, "text encoder: the first forward of a larger batch allocates its workspace and cannot run "
                                               "under stream capture -- run it eagerly once, then capture");
    TRY(t.ar.ensure(need));
    char* p = t.ar.base;
    float* xa = (float*)p; p += b_x;
    float* xb = (float*)p; p += b_x;
    half_t* h16 = (half_t*)p; p += b_h;
    half_t* ao = (half_t*)p; p += b_h;
    half_t* qkv = (half_t*)p; p += b_qkv;
    half_t* ff = (half_t*)p;
    const size_t esz = odt == DT_F32 ? 4 : 2;
    auto snap = [&](int k, const float* x) -> int {     // hidden_states[k] = the stream after k layers
        if (!hidden) return 0;
        return op_text_store(x, (char*)hidden + (size_t)k * M * C * esz, odt, (size_t)M * C, s);
    };
    TRY(op_text_embed(ids, t.tok, t.pos, c.vocab_size, N, L, C, xa, t.layers[0].ln1.g, t.layers[0].ln1.b, eps, h16, t.bad, s));
    TRY(snap(0, xa));
    const float scale = 1.0f / std::sqrt(64.0f);
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        const TextLayer& l = t.layers[i];
        TRY(linear(l.qkv, h16, qkv, DT_F16, M, nullptr, 0, s));
        TRY(op_text_attn(qkv, 3L * C, ao, C, N, L, c.num_attention_heads, scale, s));
        TRY(linear(l.out, ao, xb, DT_F32, M, xa, 0, s));
        TRY(op_layernorm(xb, DT_F32, C, l.ln2.g, l.ln2.b, h16, C, M, C, eps, s));
        TRY(linear(l.fc1, h16, ff, DT_F16, M, nullptr, 2, s));
        TRY(linear(l.fc2, ff, xa, DT_F32, M, xb, 0, s));
        TRY(snap(i + 1, xa));
        if (i + 1 < c.num_hidden_layers)
            TRY(op_layernorm(xa, DT_F32, C, t.layers[i + 1].ln1.g, t.layers[i + 1].ln1.b, h16, C, M, C, eps, s));
    }
    if (last || pooled)
        TRY(op_text_final(xa, DT_F32, M, C, t.final_ln.g, t.final_ln.b, eps, last, odt, ids, L, c.eos_token_id, pooled, s));
    return t.leave(s, capturing);
}

}  // namespace

#define S(stream) ((hipStream_t)(stream))

extern "C" {

int ctrl_text_encoder_create(const ctrl_text_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                             ctrl_text_encoder** out) {
    CTRL_CHECK(cfg && out && (tensors || n_tensors == 0), "text_encoder_create: null argument");
    *out = nullptr;
    TRY(validate(*cfg));
    TextEncoder* t = new TextEncoder();
    t->cfg = *cfg;
    int rc = t->init_base(n_tensors ? tensors[0].data : nullptr);
    DeviceGuard dg(t->device);
    if (!rc) {
        t->pk = new Packer(tensors, n_tensors, S(stream));
        rc = build_text(*t->pk, *t);
        if (!rc) rc = t->pk->finish();
    }
    if (!rc && hipMalloc((void**)&t->bad, sizeof(int)) != hipSuccess) { ctrl_set_error("text_encoder_create: hipMalloc failed"); rc = 1; }
    if (!rc && hipMemset(t->bad, 0, sizeof(int)) != hipSuccess) { ctrl_set_error("text_encoder_create: hipMemset failed"); rc = 1; }
    if (rc) { delete t; return rc; }
    *out = (ctrl_text_encoder*)t;
    return 0;
}

void ctrl_text_encoder_destroy(ctrl_text_encoder* h) {
    if (!h) return;
    TextEncoder* t = (TextEncoder*)h;
    DeviceGuard dg(t->device);
    (void)hipDeviceSynchronize();        // queued launches and captured graphs may still address the workspace
    delete t;
}

int ctrl_text_encoder_forward(ctrl_text_encoder* h, const int64_t* input_ids, int N, int L, void* last_hidden, void* pooled,
                              void* hidden_states, int out_dtype, void* stream) {
    CTRL_CHECK(h != nullptr, "text_encoder_forward: null plan");
    TextEncoder* t = (TextEncoder*)h;
    DeviceGuard dg(t->device);
    return forward(*t, input_ids, N, L, last_hidden, pooled, hidden_states, out_dtype, S(stream));
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

}  // extern "C"
