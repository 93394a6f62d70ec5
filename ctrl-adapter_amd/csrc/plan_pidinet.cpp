// PiDiNet annotator plan (controlnet_aux PidiNetDetector over pidinet(): the reference's `softedge` condition, model/ctrl_helper.py:103-107,
// 184-185).  Per group of frames:
//   stem | fifteen fused PDC blocks (one launch each) | behind every stage its context head (reduce, context, side map) | the fuse |
//   with scribble HED's three tail kernels (hed.hip).
// At creation every pixel-difference weight is turned into its vanilla 3x3 / 5x5 kernel on the host (pidi_convert_pdc: double, rounded
// once) and every weight is padded to the kernels' channel widths (60 -> 64, 120 -> 128, 240 -> 256; the pads are zeros).
// fp16 activations ping-pong between two buffers of one group's largest map; no launch looks across frames and every sum has a fixed
// order, so a frame's result does not depend on its batch or group.
#include "plan_common.h"
#include <cmath>

namespace {

constexpr int kStages = 4, kLayers = 16;
constexpr int kW[kStages] = {60, 120, 240, 240}, kBlocksOf[kStages] = {3, 4, 4, 4};
constexpr int kKindOf[4] = {1, 2, 3, 0};            // carv4: layer L is cd, ad, rd, cv by L % 4 (pidi_convert_pdc's codes)
constexpr size_t kDefaultCap = (size_t)1 << 30;

struct PidiBlock {
    int cin = 0, cout = 0, kind = 0, taps = 9;
    bool pool = false;
    float *r_c1 = nullptr, *r_c2 = nullptr, *r_sw = nullptr, *r_sb = nullptr;      // as loaded (device fp32)
    float* dw = nullptr; half_t* w2 = nullptr; half_t* wsc = nullptr; float* bsc = nullptr;
};
struct PidiHead {
    int C = 0;
    float *r_c1w = nullptr, *r_c1b = nullptr, *r_c2[4] = {}, *r_a1w = nullptr, *r_a1b = nullptr, *r_a2w = nullptr, *r_rw = nullptr, *r_rb = nullptr;
    half_t* w1 = nullptr; float* b1 = nullptr; half_t* wd = nullptr;
    float par[124] = {}, side[37] = {};
};
struct Pidi : StandalonePlan {
    ctrl_pidi_config cfg{};
    float* r_init = nullptr;
    float* stem_w = nullptr;
    PidiBlock blk[kLayers - 1];
    PidiHead head[kStages];
    float *r_clw = nullptr, *r_clb = nullptr;
    float cls[5] = {};
    int32_t* flag = nullptr;       // raised by a launch that writes an fp16 value outside the format's range
};

int validate(const ctrl_pidi_config& c) {
    CTRL_CHECK(c.ws_cap_bytes >= 0, "pidi: ws_cap_bytes must not be negative (0 = the default, 1 GiB)");
    CTRL_CHECK(c.frames_per_group >= 0, "pidi: frames_per_group must be 0 (sized from the workspace cap) or positive");
    return 0;
}

int build_pidi(ParamSink& ps, Pidi& t) {
    TRY(ps.raw_f32("init_block.weight", {kW[0], 3, 3, 3}, &t.r_init));
    int L = 1, cin = kW[0];
    for (int s = 0; s < kStages; ++s)
        for (int j = 0; j < kBlocksOf[s]; ++j, ++L) {
            PidiBlock& b = t.blk[L - 1];
            const std::string pre = "block" + std::to_string(s + 1) + "_" + std::to_string(j + 1) + ".";
            b.cin = cin; b.cout = kW[s]; b.kind = kKindOf[L % 4]; b.taps = b.kind == 3 ? 25 : 9; b.pool = s > 0 && j == 0;
            TRY(ps.raw_f32(pre + "conv1.weight", {b.cin, 1, 3, 3}, &b.r_c1));
            TRY(ps.raw_f32(pre + "conv2.weight", {b.cout, b.cin, 1, 1}, &b.r_c2));
            if (b.pool) {
                TRY(ps.raw_f32(pre + "shortcut.weight", {b.cout, b.cin, 1, 1}, &b.r_sw));
                TRY(ps.raw_f32(pre + "shortcut.bias", {b.cout}, &b.r_sb));
            }
            cin = b.cout;
        }
    for (int i = 0; i < kStages; ++i) {
        PidiHead& h = t.head[i];
        h.C = kW[i];
        const std::string di = "dilations." + std::to_string(i) + ".", at = "attentions." + std::to_string(i) + ".",
                          cr = "conv_reduces." + std::to_string(i) + ".conv.";
        TRY(ps.raw_f32(di + "conv1.weight", {kPidiHeadC, h.C, 1, 1}, &h.r_c1w));
        TRY(ps.raw_f32(di + "conv1.bias", {kPidiHeadC}, &h.r_c1b));
        for (int k = 0; k < 4; ++k) TRY(ps.raw_f32(di + "conv2_" + std::to_string(k + 1) + ".weight", {kPidiHeadC, kPidiHeadC, 3, 3}, &h.r_c2[k]));
        TRY(ps.raw_f32(at + "conv1.weight", {4, kPidiHeadC, 1, 1}, &h.r_a1w));
        TRY(ps.raw_f32(at + "conv1.bias", {4}, &h.r_a1b));
        TRY(ps.raw_f32(at + "conv2.weight", {1, 4, 3, 3}, &h.r_a2w));
        TRY(ps.raw_f32(cr + "weight", {1, kPidiHeadC, 1, 1}, &h.r_rw));
        TRY(ps.raw_f32(cr + "bias", {1}, &h.r_rb));
    }
    TRY(ps.raw_f32("classifier.weight", {1, kStages, 1, 1}, &t.r_clw));
    TRY(ps.raw_f32("classifier.bias", {1}, &t.r_clb));
    return 0;
}

int fetch(const float* dev, size_t n, std::vector<float>* out) {
    out->resize(n);
    HIP_TRY(hipMemcpy(out->data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int upload(Pidi& t, const void* host, size_t bytes, void** dev) {
    TRY(t.pk->dalloc(bytes, dev));
    HIP_TRY(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// [rows][cols] fp32 -> fp16 [rows_p][cols_p], zero padded; a value outside the fp16 range is refused
int pad_f16(const std::vector<float>& w, int rows, int cols, int rows_p, int cols_p, std::vector<half_t>* out) {
    out->assign((size_t)rows_p * cols_p, (half_t)0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const float v = w[(size_t)r * cols + c];
            CTRL_CHECK(std::fabs(v) <= 65504.0f, "pidi: a weight tensor holds values outside the fp16 range (|w| > 65504, inf or nan): the MFMA "
                                                 "operand format of this library cannot represent this checkpoint");
            (*out)[(size_t)r * cols_p + c] = (half_t)v;
        }
    return 0;
}

// after the raw copies: everything converted and padded on the host, then uploaded
int finish_build(Pidi& t, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<float> a, b, c;
    std::vector<half_t> h;
    {   // stem: the `cd` conversion, then [tap][cin][64]
        TRY(fetch(t.r_init, (size_t)kW[0] * 27, &a));
        b.resize(a.size());
        TRY(pidi_convert_pdc(1, a.data(), kW[0], 3, b.data()));
        c.assign(27 * 64, 0.f);
        for (int co = 0; co < kW[0]; ++co)
            for (int ci = 0; ci < 3; ++ci)
                for (int k = 0; k < 9; ++k) c[(k * 3 + ci) * 64 + co] = b[(co * 3 + ci) * 9 + k];
        TRY(upload(t, c.data(), c.size() * sizeof(float), (void**)&t.stem_w));
    }
    for (PidiBlock& bl : t.blk) {
        const int cip = pidi_cp(bl.cin), cop = pidi_cp(bl.cout);
        TRY(fetch(bl.r_c1, (size_t)bl.cin * 9, &a));
        b.resize((size_t)bl.cin * bl.taps);
        TRY(pidi_convert_pdc(bl.kind, a.data(), bl.cin, 1, b.data()));
        c.assign((size_t)bl.taps * cip, 0.f);
        for (int ch = 0; ch < bl.cin; ++ch)
            for (int k = 0; k < bl.taps; ++k) c[(size_t)k * cip + ch] = b[(size_t)ch * bl.taps + k];
        TRY(upload(t, c.data(), c.size() * sizeof(float), (void**)&bl.dw));
        TRY(fetch(bl.r_c2, (size_t)bl.cout * bl.cin, &a));
        TRY(pad_f16(a, bl.cout, bl.cin, cop, cip, &h));
        TRY(upload(t, h.data(), h.size() * sizeof(half_t), (void**)&bl.w2));
        if (bl.pool) {
            TRY(fetch(bl.r_sw, (size_t)bl.cout * bl.cin, &a));
            TRY(pad_f16(a, bl.cout, bl.cin, cop, cip, &h));
            TRY(upload(t, h.data(), h.size() * sizeof(half_t), (void**)&bl.wsc));
            TRY(fetch(bl.r_sb, bl.cout, &a));
            a.resize(cop, 0.f);
            TRY(upload(t, a.data(), a.size() * sizeof(float), (void**)&bl.bsc));
        }
    }
    for (PidiHead& hd : t.head) {
        const int cp = pidi_cp(hd.C);
        TRY(fetch(hd.r_c1w, (size_t)kPidiHeadC * hd.C, &a));
        TRY(pad_f16(a, kPidiHeadC, hd.C, kPidiHeadCP, cp, &h));
        TRY(upload(t, h.data(), h.size() * sizeof(half_t), (void**)&hd.w1));
        TRY(fetch(hd.r_c1b, kPidiHeadC, &a));
        a.resize(kPidiHeadCP, 0.f);
        TRY(upload(t, a.data(), a.size() * sizeof(float), (void**)&hd.b1));
        std::vector<half_t> wd((size_t)kPidiHeadTaps * kPidiHeadCP * kPidiHeadCP, (half_t)0);
        for (int k = 0; k < 4; ++k) {
            TRY(fetch(hd.r_c2[k], (size_t)kPidiHeadC * kPidiHeadC * 9, &a));
            for (int co = 0; co < kPidiHeadC; ++co)
                for (int ci = 0; ci < kPidiHeadC; ++ci)
                    for (int tp = 0; tp < 9; ++tp) {
                        const float v = a[((size_t)co * kPidiHeadC + ci) * 9 + tp];
                        CTRL_CHECK(std::fabs(v) <= 65504.0f, "pidi: a dilated convolution's weight lies outside the fp16 range");
                        wd[((size_t)(k * 9 + tp) * kPidiHeadCP + co) * kPidiHeadCP + ci] = (half_t)v;
                    }
        }
        TRY(upload(t, wd.data(), wd.size() * sizeof(half_t), (void**)&hd.wd));
        TRY(fetch(hd.r_a1w, 4 * kPidiHeadC, &a));
        for (int i = 0; i < 96; ++i) hd.par[i] = a[i];
        TRY(fetch(hd.r_a1b, 4, &a));
        for (int i = 0; i < 4; ++i) hd.par[96 + i] = a[i];
        TRY(fetch(hd.r_rw, kPidiHeadC, &a));
        for (int i = 0; i < kPidiHeadC; ++i) hd.par[100 + i] = a[i];
        TRY(fetch(hd.r_a2w, 36, &a));                 // [1][4][3][3] -> [ky][kx][4]
        for (int ch = 0; ch < 4; ++ch)
            for (int tp = 0; tp < 9; ++tp) hd.side[tp * 4 + ch] = a[ch * 9 + tp];
        TRY(fetch(hd.r_rb, 1, &a));
        hd.side[36] = a[0];
    }
    TRY(fetch(t.r_clw, kStages, &a));
    for (int i = 0; i < kStages; ++i) t.cls[i] = a[i];
    TRY(fetch(t.r_clb, 1, &a));
    t.cls[4] = a[0];
    TRY(t.pk->dalloc(256, (void**)&t.flag));
    HIP_TRY(hipMemset(t.flag, 0, 256));
    return 0;
}

struct PidiFwd {
    const unsigned char* src; int N, H, W, scribble, filter, ch;
    unsigned char* out; float* logits;
};

// frames [f0, f0 + n) of the call
int run_group(Ctx& cx, const Pidi& t, const PidiFwd& a, int f0, int n) {
    const size_t HW = (size_t)a.H * a.W;
    half_t* x = cx.h((size_t)n * HW * 64);
    half_t* y = cx.h((size_t)n * HW * 64);
    half_t* tb = cx.h((size_t)n * HW * kPidiHeadCP);
    float *a4[kStages], *d[kStages], *e[kStages];
    for (int i = 0; i < kStages; ++i) {
        a4[i] = cx.f((size_t)n * (HW >> (2 * i)) * 4);
        d[i] = cx.f((size_t)n * (HW >> (2 * i)));
        e[i] = cx.f((size_t)n * (HW >> (2 * i)));
    }
    RUN(cx, op_pidi_stem(a.src + (size_t)f0 * HW * 3, n, a.H, a.W, t.stem_w, x, t.flag, cx.s));
    int h = a.H, w = a.W, L = 0;
    for (int i = 0; i < kStages; ++i) {
        for (int j = 0; j < kBlocksOf[i]; ++j, ++L) {
            const PidiBlock& b = t.blk[L];
            RUN(cx, op_pidi_block(x, n, h, w, b.cin, b.cout, b.taps, b.dw, b.w2, b.wsc, b.bsc, b.pool ? 1 : 0, y, t.flag, cx.s));
            std::swap(x, y);
            if (b.pool) { h /= 2; w /= 2; }
        }
        const PidiHead& hd = t.head[i];
        RUN(cx, op_pidi_head_reduce(x, n, h, w, hd.C, hd.w1, hd.b1, tb, t.flag, cx.s));
        RUN(cx, op_pidi_head_context(tb, n, h, w, hd.wd, hd.par, a4[i], d[i], cx.s));
        RUN(cx, op_pidi_side(a4[i], d[i], n, h, w, hd.side, e[i], cx.s));
    }
    float* lg = a.logits ? a.logits + (size_t)f0 * HW : nullptr;
    if (!a.scribble) {
        RUN(cx, op_pidi_fuse(e, n, a.H, a.W, t.cls, a.filter, a.ch, a.out + (size_t)f0 * HW * a.ch, lg, cx.s));
        return 0;
    }
    unsigned char* soft = (unsigned char*)cx.alloc((size_t)n * HW);
    float* blurred = cx.f((size_t)n * HW);
    unsigned char* thin = (unsigned char*)cx.alloc((size_t)n * HW);
    RUN(cx, op_pidi_fuse(e, n, a.H, a.W, t.cls, a.filter, 1, soft, lg, cx.s));
    RUN(cx, op_hed_blur_f32(soft, n, a.H, a.W, blurred, cx.s));
    RUN(cx, op_hed_nms(blurred, n, a.H, a.W, thin, cx.s));
    RUN(cx, op_hed_blur_u8_bin(thin, n, a.H, a.W, a.ch, a.out + (size_t)f0 * HW * a.ch, cx.s));
    return 0;
}

int check_args(const PidiFwd& a, int fpg) {
    CTRL_CHECK(a.N >= 1, "pidi: at least one frame is required");
    CTRL_CHECK(a.H >= 64 && a.W >= 64 && a.H % 64 == 0 && a.W % 64 == 0 && a.H <= 4096 && a.W <= 4096,
               "pidi: H and W must be multiples of 64 (what PidiNetDetector's resize_image produces), at most 4096");
    CTRL_CHECK(a.ch == 1 || a.ch == 3, "pidi: out_channels must be 1 or 3");
    CTRL_CHECK(fpg >= 0, "pidi: frames_per_group must be 0 (sized from the workspace cap) or positive");
    return 0;
}

size_t dry_bytes(const Pidi& t, const PidiFwd& a, int n) {
    Arena tmp;
    Ctx dry{&tmp, nullptr, true};
    (void)run_group(dry, t, a, 0, n);
    return tmp.peak + 1024;
}

// frames per group: the caller's, the plan's, or equal groups of the largest size below the cap; always within the 2^31-element index
// rule of the launches (n * H * W * 64 elements in the widest map)
int group_size(const Pidi& t, const PidiFwd& a, int fpg) {
    const double lim = std::floor((2147483648.0 - 1.0) / ((double)a.H * a.W * 64));
    const int idx_max = (int)std::min(lim, 4096.0);
    if (idx_max < 1) return 0;
    if (fpg <= 0) fpg = t.cfg.frames_per_group;
    if (fpg > 0) return std::min(std::min(fpg, a.N), idx_max);
    const size_t cap = t.cfg.ws_cap_bytes > 0 ? (size_t)t.cfg.ws_cap_bytes : kDefaultCap;
    const size_t one = dry_bytes(t, a, 1);
    const int gmax = (int)std::max<size_t>(1, std::min<size_t>(cap / one, (size_t)idx_max));
    const int groups = (a.N + gmax - 1) / gmax;
    return (a.N + groups - 1) / groups;
}

int forward(Pidi& t, const PidiFwd& a, int fpg, hipStream_t s) {
    CTRL_CHECK(a.src != nullptr && a.out != nullptr, "pidi: frames and out are required");
    TRY(check_args(a, fpg));
    CTRL_CHECK(((uintptr_t)a.out & 3) == 0, "pidi: out must be 4-byte aligned");
    const int g = group_size(t, a, fpg);
    CTRL_CHECK(g >= 1, "pidi: the frame is too large for one launch");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    CTRL_CHECK(!capturing, "pidi: the stream is capturing; the forward reads its fp16 range flag back at the end and cannot be recorded "
                           "into a graph");
    TRY(t.reserve(dry_bytes(t, a, g), false, "pidi", "group of frames"));
    HIP_TRY(hipMemsetAsync(t.flag, 0, sizeof(int32_t), s));
    Ctx cx{&t.ar, s, false};
    for (int f0 = 0; f0 < a.N; f0 += g) {
        t.ar.off = 0;
        TRY(run_group(cx, t, a, f0, std::min(g, a.N - f0)));
    }
    int32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, t.flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    TRY(t.leave(s, false));
    CTRL_CHECK(bad == 0, "pidi: an activation left the fp16 range (|x| > 65504) -- the output is not valid");
    return 0;
}

}  // namespace

extern "C" {

int ctrl_pidi_create(const ctrl_pidi_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_pidi** out) {
    return plan_create<Pidi>("pidi_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_pidi, finish_build);
}

void ctrl_pidi_destroy(ctrl_pidi* h) { plan_destroy<Pidi>(h); }

int ctrl_pidi_forward(ctrl_pidi* h, const void* frames_u8, int N, int H, int W, int scribble, int apply_filter, int out_channels, void* out_u8,
                      float* logits, int frames_per_group, void* stream) {
    CTRL_CHECK(h != nullptr, "pidi_forward: null plan");
    Pidi* t = (Pidi*)h;
    DeviceGuard dg(t->device);
    const PidiFwd a = {(const unsigned char*)frames_u8, N, H, W, scribble ? 1 : 0, apply_filter ? 1 : 0, out_channels, (unsigned char*)out_u8, logits};
    return forward(*t, a, frames_per_group, S(stream));
}

int64_t ctrl_pidi_ws_bytes(ctrl_pidi* h, int N, int H, int W, int scribble, int frames_per_group) {
    if (!h) return 0;
    const Pidi* t = (const Pidi*)h;
    const PidiFwd a = {nullptr, N, H, W, scribble ? 1 : 0, 0, 3, nullptr, nullptr};
    if (check_args(a, frames_per_group)) return 0;
    const int g = group_size(*t, a, frames_per_group);
    return g >= 1 ? (int64_t)dry_bytes(*t, a, g) : 0;
}

int ctrl_pidi_convert_pdc(int kind, const float* w, int Co, int Ci, float* out) { return pidi_convert_pdc(kind, w, Co, Ci, out); }

int ctrl_pidi_launch_shape(int kernel, int* tile_h, int* tile_w) {
    CTRL_CHECK(tile_h && tile_w && (kernel == 0 || kernel == 1), "pidi_launch_shape: kernel must be 0 (block) or 1 (context head)");
    pidi_launch_shape(kernel, tile_h, tile_w);
    return 0;
}

int ctrl_op_pidi_stem(const void* src_u8, int N, int H, int W, const float* w, void* out_f16, int32_t* nonfinite, void* stream) {
    return op_pidi_stem((const unsigned char*)src_u8, N, H, W, w, (half_t*)out_f16, nonfinite, S(stream));
}
int ctrl_op_pidi_block(const void* x_f16, int N, int H, int W, int Cin, int Cout, int taps, const float* dw, const void* w2_f16,
                       const void* wsc_f16, const float* bsc, int pool, void* out_f16, int32_t* nonfinite, void* stream) {
    return op_pidi_block((const half_t*)x_f16, N, H, W, Cin, Cout, taps, dw, (const half_t*)w2_f16, (const half_t*)wsc_f16, bsc, pool,
                         (half_t*)out_f16, nonfinite, S(stream));
}
int ctrl_op_pidi_head_reduce(const void* x_f16, int N, int H, int W, int C, const void* w1_f16, const float* b1, void* t_f16,
                             int32_t* nonfinite, void* stream) {
    return op_pidi_head_reduce((const half_t*)x_f16, N, H, W, C, (const half_t*)w1_f16, b1, (half_t*)t_f16, nonfinite, S(stream));
}
int ctrl_op_pidi_head_context(const void* t_f16, int N, int H, int W, const void* wd_f16, const float* par_host124, float* a4, float* d,
                              void* stream) {
    return op_pidi_head_context((const half_t*)t_f16, N, H, W, (const half_t*)wd_f16, par_host124, a4, d, S(stream));
}
int ctrl_op_pidi_side(const float* a4, const float* d, int N, int H, int W, const float* par_host37, float* e, void* stream) {
    return op_pidi_side(a4, d, N, H, W, par_host37, e, S(stream));
}
int ctrl_op_pidi_fuse(const float* const* maps, int N, int H, int W, const float* par_host5, int apply_filter, int out_channels,
                      void* out_u8, float* logits, void* stream) {
    return op_pidi_fuse(maps, N, H, W, par_host5, apply_filter, out_channels, (unsigned char*)out_u8, logits, S(stream));
}

}  // extern "C"
