// Lineart annotator plan (controlnet_aux LineartDetector over Generator(3, 1, 3): the reference's `lineart` condition,
// model/ctrl_helper.py:111-114, 190-191).  Per group of frames:
//   stem (uint8 frame -> reflect-3 7x7 conv) | InstanceNorm + ReLU | two stride-2 3x3 convolutions on the implicit GEMM, each with its
//   InstanceNorm + ReLU | three residual blocks: the producer's InstanceNorm writes its output REFLECT-PADDED by 1, so both 3x3 convolutions run
//   as VALID convolutions over the padded operand (tap_origin = 1, stride 1, Hin = Hout + 2), the second norm adds the block's input |
//   two ConvTranspose2d(3, stride 2) as the implicit GEMM's four-phase form with a transposed weight pack (16/9 of the minimal FLOPs, against
//   4x for zero insertion), each with its InstanceNorm + ReLU, the last one reflect-padded by 3 | the head (7x7 conv to one channel, sigmoid,
//   inverted uint8).
// Every norm is affine-free InstanceNorm, so the bias of every convolution in front of one cancels: only model4.1's is kept (the others must
// still be present and well-shaped).  fp16 activations rotate through three buffers of one group's largest map; no launch looks across
// frames, no GEMM is split along K and the statistics are reduced in a fixed order, so a frame's result does not depend on its batch or group.
// Both generators (fine, and coarse when given) are packed into the one plan; `coarse` is an argument of the forward.
#include "plan_common.h"
#include <cmath>

namespace {

constexpr int kResBlocks = 3;
constexpr float kEps = 1e-5f;
constexpr size_t kDefaultCap = (size_t)1 << 30;

struct Gen {
    float *r_stem = nullptr, *r_head = nullptr, *r_head_b = nullptr;      // as loaded (device fp32)
    float *stem_w = nullptr, *head_w = nullptr;                           // [49][3][64], [49][64]
    float head_b = 0.f;
    ConvW down[2], res[2 * kResBlocks];
    half_t* up[2] = {nullptr, nullptr};                                   // phase packs of model3.0, model3.3
};
struct Lineart : StandalonePlan {
    ctrl_lineart_config cfg{};
    Gen gen[2];                    // fine, coarse
    int32_t* flag = nullptr;       // raised by a launch that writes an fp16 value outside the format's range
};

int validate(const ctrl_lineart_config& c) {
    CTRL_CHECK(c.ws_cap_bytes >= 0, "lineart: ws_cap_bytes must not be negative (0 = the default, 1 GiB)");
    CTRL_CHECK(c.frames_per_group >= 0, "lineart: frames_per_group must be 0 (sized from the workspace cap) or positive");
    CTRL_CHECK(c.has_coarse == 0 || c.has_coarse == 1, "lineart: has_coarse must be 0 or 1");
    return 0;
}

int build_gen(Packer& pk, const std::string& pre, Gen& g) {
    float* dropped = nullptr;
    TRY(pk.raw_f32(pre + "model0.1.weight", {64, 3, 7, 7}, &g.r_stem));
    TRY(pk.raw_f32(pre + "model0.1.bias", {64}, &dropped));
    TRY(pk.conv(pre + "model1.0", 128, 64, 3, false, &g.down[0], false, false));
    TRY(pk.conv(pre + "model1.3", 256, 128, 3, false, &g.down[1], false, false));
    for (int b = 0; b < kResBlocks; ++b)
        for (int j = 0; j < 2; ++j)
            TRY(pk.conv(pre + "model2." + std::to_string(b) + ".conv_block." + (j ? "5" : "1"), 256, 256, 3, false, &g.res[2 * b + j], false, false));
    const int cin[2] = {256, 128}, cout[2] = {128, 64};
    for (int k = 0; k < 2; ++k) {
        const std::string name = pre + (k ? "model3.3" : "model3.0");
        const ctrl_tensor_ref *w, *b;
        TRY(pk.get(name + ".weight", {cin[k], cout[k], 3, 3}, &w));
        TRY(pk.get(name + ".bias", {cout[k]}, &b));
        TRY(pk.dalloc((size_t)16 * cin[k] * cout[k] * sizeof(half_t), (void**)&g.up[k]));
        TRY(op_pack_convT_w_phase(w->data, w->dtype, g.up[k], cin[k], cout[k], pk.s, pk.ovf_flag()));
    }
    TRY(pk.raw_f32(pre + "model4.1.weight", {1, 64, 7, 7}, &g.r_head));
    TRY(pk.raw_f32(pre + "model4.1.bias", {1}, &g.r_head_b));
    return 0;
}

int build_lineart(Packer& pk, Lineart& t) {
    TRY(build_gen(pk, "fine.", t.gen[0]));
    if (t.cfg.has_coarse) TRY(build_gen(pk, "coarse.", t.gen[1]));
    return 0;
}

int fetch(const float* dev, size_t n, std::vector<float>* out) {
    out->resize(n);
    HIP_TRY(hipMemcpy(out->data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int upload(Lineart& t, const void* host, size_t bytes, void** dev) {
    TRY(t.pk->dalloc(bytes, dev));
    HIP_TRY(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// after the raw copies: the two 7x7 weights in the tap-major order of their kernels
int finish_build(Lineart& t, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<float> a, c;
    for (int gi = 0; gi < (t.cfg.has_coarse ? 2 : 1); ++gi) {
        Gen& g = t.gen[gi];
        TRY(fetch(g.r_stem, 64 * 3 * 49, &a));
        c.assign(49 * 3 * 64, 0.f);
        for (int co = 0; co < 64; ++co)
            for (int ci = 0; ci < 3; ++ci)
                for (int k = 0; k < 49; ++k) c[(k * 3 + ci) * 64 + co] = a[(co * 3 + ci) * 49 + k];
        TRY(upload(t, c.data(), c.size() * sizeof(float), (void**)&g.stem_w));
        TRY(fetch(g.r_head, 64 * 49, &a));
        c.assign(49 * 64, 0.f);
        for (int ci = 0; ci < 64; ++ci)
            for (int k = 0; k < 49; ++k) c[k * 64 + ci] = a[ci * 49 + k];
        TRY(upload(t, c.data(), c.size() * sizeof(float), (void**)&g.head_w));
        TRY(fetch(g.r_head_b, 1, &a));
        g.head_b = a[0];
    }
    TRY(t.pk->dalloc(256, (void**)&t.flag));
    HIP_TRY(hipMemset(t.flag, 0, 256));
    return 0;
}

struct LineFwd {
    const unsigned char* src; int N, H, W, coarse, ch;
    unsigned char* out; float* logits;
};

// a bias-free 3x3 convolution on the implicit GEMM: padding 1 (tap_origin 0) or valid over a padded operand (tap_origin 1, stride 1)
int conv3(Ctx& cx, const Lineart& t, const half_t* x, const ConvW& c, int n, int Hin, int Win, int Hout, int Wout, int stride, int tap_origin,
          half_t* y) {
    IGemmArgs g = {};
    g.A = x; g.lda = c.Cin; g.mode = IG_CONV2D; g.Cin = c.Cin; g.taps = 9;
    g.Hin = Hin; g.Win = Win; g.Hout = Hout; g.Wout = Wout; g.stride = stride; g.up = 1; g.tap_origin = tap_origin;
    g.W = c.w; g.M = n * Hout * Wout; g.Nout = c.Cout; g.Ktot = 9 * c.Cin;
    g.rows_per_img = Hout * Wout; g.scale = 1.f;
    g.nseg = 1;
    g.seg[0] = IGemmSeg{y, c.Cout, 0, c.Cout, SEG_ROW, DT_F16, 1, 0};
    g.nonfinite = t.flag;
    RUN(cx, op_igemm(g, cx.s));
    return 0;
}

// ConvTranspose2d(3, stride 2, padding 1, output_padding 1) as the four-phase form over the source grid
int convT(Ctx& cx, const Lineart& t, const half_t* x, const half_t* wp, int n, int Hin, int Win, int Cin, int Cout, half_t* y) {
    IGemmArgs g = {};
    g.A = x; g.lda = Cin; g.mode = IG_CONV2D_PHASE; g.Cin = Cin; g.taps = 4;
    g.Hin = Hin; g.Win = Win; g.Hout = 2 * Hin; g.Wout = 2 * Win; g.stride = 1; g.up = 2;
    g.W = wp; g.M = n * 4 * Hin * Win; g.Nout = Cout; g.Ktot = 4 * Cin;
    g.rows_per_img = 4 * Hin * Win; g.scale = 1.f;
    g.nseg = 1;
    g.seg[0] = IGemmSeg{y, Cout, 0, Cout, SEG_ROW, DT_F16, 1, 0};
    g.nonfinite = t.flag;
    RUN(cx, op_igemm(g, cx.s));
    return 0;
}

struct NormWs { float* stats; float* part; };
int inorm(Ctx& cx, const Lineart& t, const NormWs& ws, const half_t* x, int n, int H, int W, int C, int relu, const half_t* res, int pad,
          half_t* y) {
    RUN(cx, op_in_stats(x, n, H * W, C, ws.stats, ws.part, cx.s));
    RUN(cx, op_in_apply(x, ws.stats, n, H, W, C, kEps, relu, res, 1, pad, y, t.flag, cx.s));
    return 0;
}

// frames [f0, f0 + n) of the call
int run_group(Ctx& cx, const Lineart& t, const LineFwd& a, int f0, int n) {
    const Gen& g = t.gen[a.coarse ? 1 : 0];
    const int H = a.H, W = a.W, h2 = H / 2, w2 = W / 2, h = H / 4, w = W / 4;
    const size_t big = (size_t)n * (H + 6) * (W + 6) * 64;
    half_t* x = cx.h(big);
    half_t* p = cx.h(big);
    half_t* q = cx.h(big);
    NormWs ws;
    ws.stats = cx.f((size_t)n * 256 * 2);
    ws.part = cx.f(std::max(std::max(op_in_stats_ws_floats(n, H * W, 64), op_in_stats_ws_floats(n, h2 * w2, 128)),
                            op_in_stats_ws_floats(n, h * w, 256)));
    RUN(cx, op_lineart_stem(a.src + (size_t)f0 * H * W * 3, n, H, W, g.stem_w, p, t.flag, cx.s));
    TRY(inorm(cx, t, ws, p, n, H, W, 64, 1, nullptr, 0, x));
    TRY(conv3(cx, t, x, g.down[0], n, H, W, h2, w2, 2, 0, p));
    TRY(inorm(cx, t, ws, p, n, h2, w2, 128, 1, nullptr, 0, x));
    TRY(conv3(cx, t, x, g.down[1], n, h2, w2, h, w, 2, 0, p));
    TRY(inorm(cx, t, ws, p, n, h, w, 256, 1, nullptr, 1, x));
    for (int b = 0; b < kResBlocks; ++b) {         // x: the block's input, reflect-padded by 1; p, q free
        TRY(conv3(cx, t, x, g.res[2 * b], n, h + 2, w + 2, h, w, 1, 1, p));
        TRY(inorm(cx, t, ws, p, n, h, w, 256, 1, nullptr, 1, q));
        TRY(conv3(cx, t, q, g.res[2 * b + 1], n, h + 2, w + 2, h, w, 1, 1, p));
        TRY(inorm(cx, t, ws, p, n, h, w, 256, 0, x, b + 1 < kResBlocks ? 1 : 0, q));
        std::swap(x, q);
    }
    TRY(convT(cx, t, x, g.up[0], n, h, w, 256, 128, p));
    TRY(inorm(cx, t, ws, p, n, h2, w2, 128, 1, nullptr, 0, q));
    TRY(convT(cx, t, q, g.up[1], n, h2, w2, 128, 64, p));
    TRY(inorm(cx, t, ws, p, n, H, W, 64, 1, nullptr, 3, q));
    RUN(cx, op_lineart_head(q, n, H, W, g.head_w, g.head_b, a.ch, a.out + (size_t)f0 * H * W * a.ch,
                            a.logits ? a.logits + (size_t)f0 * H * W : nullptr, cx.s));
    return 0;
}

int check_args(const Lineart& t, const LineFwd& a, int fpg) {
    CTRL_CHECK(a.N >= 1, "lineart: at least one frame is required");
    CTRL_CHECK(a.H >= 64 && a.W >= 64 && a.H % 64 == 0 && a.W % 64 == 0 && a.H <= 4096 && a.W <= 4096,
               "lineart: H and W must be multiples of 64 (what LineartDetector's resize_image produces), at most 4096");
    CTRL_CHECK(a.ch == 1 || a.ch == 3, "lineart: out_channels must be 1 or 3");
    CTRL_CHECK(fpg >= 0, "lineart: frames_per_group must be 0 (sized from the workspace cap) or positive");
    CTRL_CHECK(!a.coarse || t.cfg.has_coarse, "lineart: coarse was asked for, but the plan was created without the coarse generator");
    return 0;
}

size_t dry_bytes(const Lineart& t, const LineFwd& a, int n) {
    Arena tmp;
    Ctx dry{&tmp, nullptr, true};
    (void)run_group(dry, t, a, 0, n);
    return tmp.peak + 1024;
}

// frames per group: the caller's, the plan's, or equal groups of the largest size below the cap; always within the 2^31-element index
// rule of the launches (n * (H + 6) * (W + 6) * 64 elements in the widest map)
int group_size(const Lineart& t, const LineFwd& a, int fpg) {
    const double lim = std::floor((2147483648.0 - 1.0) / ((double)(a.H + 6) * (a.W + 6) * 64));
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

int forward(Lineart& t, const LineFwd& a, int fpg, hipStream_t s) {
    CTRL_CHECK(a.src != nullptr && a.out != nullptr, "lineart: frames and out are required");
    TRY(check_args(t, a, fpg));
    const int g = group_size(t, a, fpg);
    CTRL_CHECK(g >= 1, "lineart: the frame is too large for one launch");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    CTRL_CHECK(!capturing, "lineart: the stream is capturing; the forward reads its fp16 range flag back at the end and cannot be recorded "
                           "into a graph");
    TRY(t.reserve(dry_bytes(t, a, g), false, "lineart", "group of frames"));
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
    CTRL_CHECK(bad == 0, "lineart: an activation left the fp16 range (|x| > 65504) -- the output is not valid");
    return 0;
}

}  // namespace

extern "C" {

int ctrl_lineart_create(const ctrl_lineart_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_lineart** out) {
    return plan_create<Lineart>("lineart_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_lineart, finish_build);
}

void ctrl_lineart_destroy(ctrl_lineart* h) { plan_destroy<Lineart>(h); }

int ctrl_lineart_forward(ctrl_lineart* h, const void* frames_u8, int N, int H, int W, int coarse, int out_channels, void* out_u8, float* logits,
                         int frames_per_group, void* stream) {
    CTRL_CHECK(h != nullptr, "lineart_forward: null plan");
    Lineart* t = (Lineart*)h;
    DeviceGuard dg(t->device);
    const LineFwd a = {(const unsigned char*)frames_u8, N, H, W, coarse ? 1 : 0, out_channels, (unsigned char*)out_u8, logits};
    return forward(*t, a, frames_per_group, S(stream));
}

int64_t ctrl_lineart_ws_bytes(ctrl_lineart* h, int N, int H, int W, int frames_per_group) {
    if (!h) return 0;
    const Lineart* t = (const Lineart*)h;
    const LineFwd a = {nullptr, N, H, W, 0, 3, nullptr, nullptr};
    if (check_args(*t, a, frames_per_group)) return 0;
    const int g = group_size(*t, a, frames_per_group);
    return g >= 1 ? (int64_t)dry_bytes(*t, a, g) : 0;
}

int ctrl_lineart_launch_shape(int kernel, int C, int* a, int* b) {
    CTRL_CHECK(a && b && kernel >= 0 && kernel <= 2, "lineart_launch_shape: kernel must be 0 (stem), 1 (head) or 2 (in_stats)");
    CTRL_CHECK(kernel != 2 || (C >= 8 && C <= 256 && (C & (C - 1)) == 0), "lineart_launch_shape: C must be a power of two, 8 .. 256");
    lineart_launch_shape(kernel, C, a, b);
    return 0;
}

int ctrl_op_lineart_stem(const void* src_u8, int N, int H, int W, const float* w, void* out_f16, int32_t* nonfinite, void* stream) {
    return op_lineart_stem((const unsigned char*)src_u8, N, H, W, w, (half_t*)out_f16, nonfinite, S(stream));
}
int64_t ctrl_op_in_stats_ws_floats(int N, int HW, int C) { return (int64_t)op_in_stats_ws_floats(N, HW, C); }
int ctrl_op_in_stats(const void* x_f16, int N, int HW, int C, float* stats, float* ws, void* stream) {
    return op_in_stats((const half_t*)x_f16, N, HW, C, stats, ws, S(stream));
}
int ctrl_op_in_apply(const void* x_f16, const float* stats, int N, int H, int W, int C, float eps, int relu, const void* res_f16, int res_pad,
                     int pad, void* out_f16, int32_t* nonfinite, void* stream) {
    return op_in_apply((const half_t*)x_f16, stats, N, H, W, C, eps, relu, (const half_t*)res_f16, res_pad, pad, (half_t*)out_f16, nonfinite,
                       S(stream));
}
int ctrl_op_lineart_head(const void* xp_f16, int N, int H, int W, const float* w, float bias, int out_channels, void* out_u8, float* logits,
                         void* stream) {
    return op_lineart_head((const half_t*)xp_f16, N, H, W, w, bias, out_channels, (unsigned char*)out_u8, logits, S(stream));
}
int ctrl_op_pack_convt_w_phase(const void* w, int dtype, void* out, int Cin, int Cout, void* stream) {
    return op_pack_convT_w_phase(w, dtype, (half_t*)out, Cin, Cout, S(stream));
}
int ctrl_op_pack_convt_w_phase_ovf(const void* w, int dtype, void* out, int Cin, int Cout, int32_t* ovf, void* stream) {
    return op_pack_convT_w_phase(w, dtype, (half_t*)out, Cin, Cout, S(stream), ovf);
}

}  // extern "C"
