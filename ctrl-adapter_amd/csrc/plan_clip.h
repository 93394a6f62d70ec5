// The CLIP transformer tower shared by the text plan (plan_text.cpp) and the vision plan (plan_vision.cpp): the layer weights, the
// linear of the plan's GEMM form with its scratch, the hidden-state snapshot and the per-layer launch sequence.  The plans differ in
// the attention step alone (causal text kernel against V^T + flash attention), which they pass in.
#pragma once
#include "plan_common.h"
#include <algorithm>

struct ClipLayer {
    Norm ln1, ln2;
    Lin qkv, out, fc1, fc2;
};

// layers `prefix`0. .. `prefix`(n-1). of hidden size C, MLP width I (transformers' CLIPEncoderLayer keys)
inline int build_clip_layers(ParamSink& ps, const std::string& prefix, int n, int C, int I, std::vector<ClipLayer>* out) {
    out->resize(n);
    for (int i = 0; i < n; ++i) {
        const std::string pre = prefix + std::to_string(i) + ".";
        ClipLayer& l = (*out)[i];
        TRY(ps.norm(pre + "layer_norm1", C, &l.ln1));
        TRY(ps.linear_cat({pre + "self_attn.q_proj", pre + "self_attn.k_proj", pre + "self_attn.v_proj"}, {C, C, C}, C, true, &l.qkv));
        TRY(ps.linear(pre + "self_attn.out_proj", C, C, true, false, &l.out));
        TRY(ps.norm(pre + "layer_norm2", C, &l.ln2));
        TRY(ps.linear(pre + "mlp.fc1", I, C, true, false, &l.fc1));
        TRY(ps.linear(pre + "mlp.fc2", C, I, true, false, &l.fc2));
    }
    return 0;
}

// with only a hidden state k asked for, the layers after k are not run
inline int clip_layers_to_run(bool tail, int hidden_index, int num_hidden_layers) {
    return (!tail && hidden_index >= 0) ? hidden_index : num_hidden_layers;
}

// row-major linear on the pinned GEMM: y[M][N] (dtype of y) = act(x[M][K] W^T + b) (+ fp32 residual)
inline int pinned_linear(const half_t* x, const half_t* W, const float* b, int N, int K, void* y, int y_dt, int M, const float* res, int act,
                         hipStream_t s) {
    IGemmArgs g = {};
    g.A = x; g.lda = K; g.mode = IG_ROWS; g.Cin = K; g.taps = 1;
    g.W = W; g.M = M; g.Nout = N; g.Ktot = K; g.bias = b; g.scale = 1.f; g.act = act;
    g.res = res; g.ldres = N; g.res_f32 = res ? 1 : 0;
    g.nseg = 1;
    g.seg[0] = IGemmSeg{y, N, 0, N, SEG_ROW, y_dt, 1, 0, nullptr};
    return op_igemm_pinned(g, s);
}

// scratch a linear of the plan's form needs besides its output: the split-K partials (form 1) or the fp32 pre-activation of an
// exact-gelu fc1 on the pinned form (form 0: the shared implicit-GEMM epilogue has no erf; the fp32 pass applies it in the same order,
// bias -> act -> residual)
struct LinScratch { float* p = nullptr; size_t bytes = 0; };

// the linear of the plan's form (act 2 quick_gelu, 3 exact gelu)
inline int run_linear(int gemm_form, const Lin& l, const half_t* x, void* y, int y_dt, int M, const float* res, int act, const LinScratch& ws,
                      hipStream_t s) {
    if (gemm_form == 1) return op_text_gemm(x, l.w, l.b, M, l.N, l.K, act, res, y, y_dt, ws.p, ws.bytes, s);
    if (act != 3) return pinned_linear(x, l.w, l.b, l.N, l.K, y, y_dt, M, res, act, s);
    TRY(pinned_linear(x, l.w, l.b, l.N, l.K, ws.p, DT_F32, M, nullptr, 0, s));
    return op_text_gemm_finish(ws.p, 1, M, l.N, nullptr, 3, res, l.N, y, y_dt, l.N, s);
}

inline size_t lin_scratch_bytes(int gemm_form, int hidden_act, int M, size_t C, size_t I) {
    if (gemm_form == 1)
        return std::max(std::max(text_gemm_ws_bytes(M, 3 * C, C), text_gemm_ws_bytes(M, C, C)),
                        std::max(text_gemm_ws_bytes(M, I, C), text_gemm_ws_bytes(M, C, I)));
    return hidden_act == 1 ? (size_t)M * I * 4 : 0;
}

// hidden_states[k] = the stream after k layers: hidden_index -1 keeps every state in hidden [layers + 1][rows], k >= 0 state k alone
struct ClipSnapshot {
    void* hidden; int hidden_index, odt; size_t elems;       // elems: M * C of one state
    int operator()(int k, const float* x, hipStream_t s) const {
        if (!hidden || (hidden_index >= 0 && k != hidden_index)) return 0;
        const size_t slot = hidden_index >= 0 ? 0 : (size_t)k;
        return op_text_store(x, (char*)hidden + slot * elems * dt_size(odt), odt, elems, s);
    }
};

// the tower's working set, carved by the plan: two fp32 stream buffers, the fp16 LayerNorm output, the attention output, Q | K | V
// rows, the MLP hidden activation, the linears' scratch
struct ClipBufs { float* xa; float* xb; half_t* h16; half_t* ao; half_t* qkv; half_t* ff; LinScratch lws; };

// `layers` layers over the stream in b.xa, whose LN1(0) is already in b.h16; per layer: Q|K|V GEMM, attn() (b.qkv -> b.ao), out_proj
// (+ residual), LN2, fc1 (+ act), fc2 (+ residual), the snapshot, LN1 of the next layer unless this was the last one run.  The
// stream ends in b.xa.
template <class Attn>
int run_clip_layers(const std::vector<ClipLayer>& all, int layers, int gemm_form, int hidden_act, int M, int C, float eps, const ClipBufs& b,
                    const ClipSnapshot& snap, hipStream_t s, Attn attn) {
    const int fc1_act = hidden_act == 1 ? 3 : 2;
    for (int i = 0; i < layers; ++i) {
        const ClipLayer& l = all[i];
        TRY(run_linear(gemm_form, l.qkv, b.h16, b.qkv, DT_F16, M, nullptr, 0, b.lws, s));
        TRY(attn());
        TRY(run_linear(gemm_form, l.out, b.ao, b.xb, DT_F32, M, b.xa, 0, b.lws, s));
        TRY(op_layernorm(b.xb, DT_F32, C, l.ln2.g, l.ln2.b, b.h16, C, M, C, eps, s));
        TRY(run_linear(gemm_form, l.fc1, b.h16, b.ff, DT_F16, M, nullptr, fc1_act, b.lws, s));
        TRY(run_linear(gemm_form, l.fc2, b.ff, b.xa, DT_F32, M, b.xb, 0, b.lws, s));
        TRY(snap(i + 1, b.xa, s));
        if (i + 1 < layers)
            TRY(op_layernorm(b.xa, DT_F32, C, all[i + 1].ln1.g, all[i + 1].ln1.b, b.h16, C, M, C, eps, s));
    }
    return 0;
}
