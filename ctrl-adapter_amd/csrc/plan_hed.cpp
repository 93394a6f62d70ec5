// HED annotator plan (controlnet_aux ControlNetHED_Apache2 + HEDdetector: the reference's `scribble` condition,
// model/ctrl_helper.py:124-127, 196-197, and the soft-edge condition).  Per group of frames:
//   stem kernel (uint8 frame -> conv1_1 + ReLU) | the other twelve 3x3 convolutions + ReLU on the implicit GEMM (act = 3) | behind every
//   block the pool + project kernel (the pooled input of the next block, the block's fp32 side output) | the fuse kernel (bilinear,
//   mean, sigmoid, uint8) | with scribble the three tail kernels (hed.hip).
// fp16 activations ping-pong between two buffers of one group's largest map (64 channels at full resolution); a call's frames run in
// groups sized from the workspace cap.  No launch looks across frames and no GEMM is split along K (every tile form of the implicit GEMM
// walks K in the same order with the same MFMA), so a frame's result does not depend on its group.
// The trunk may run at a power-of-two scale s (ctrl_hed_config::trunk_scale): the net is positively homogeneous up to its biases.
#include "plan_common.h"
#include <cmath>

namespace {

constexpr int kBlocks = 5;
constexpr int kC[kBlocks] = {64, 128, 256, 512, 512}, kLayers[kBlocks] = {2, 2, 3, 3, 3};
constexpr size_t kDefaultCap = (size_t)1 << 30;

struct HedBlock {
    std::vector<ConvW> convs;      // the block's convolutions on the implicit GEMM (block 1: its second one)
    float* pw = nullptr;           // projection.weight [C]
    float* pb = nullptr;           // projection.bias [1]
};

struct Hed : StandalonePlan {
    ctrl_hed_config cfg{};
    float* norm = nullptr;
    float norm_host[3] = {0.f, 0.f, 0.f};
    ConvD stem;
    HedBlock blk[kBlocks];
    int32_t* flag = nullptr;       // raised by a launch that writes an fp16 value outside the format's range
};

int validate(const ctrl_hed_config& c) {
    int e = 0;
    CTRL_CHECK(c.trunk_scale > 0.f && std::isfinite(c.trunk_scale) && std::frexp(c.trunk_scale, &e) == 0.5f,
               "hed: trunk_scale must be a positive power of two");
    CTRL_CHECK(c.ws_cap_bytes >= 0, "hed: ws_cap_bytes must not be negative (0 = the default, 1 GiB)");
    return 0;
}

int build_hed(ParamSink& ps, Hed& t) {
    TRY(ps.raw_f32("norm", {1, 3, 1, 1}, &t.norm));
    int cin = 3;
    for (int k = 0; k < kBlocks; ++k) {
        const std::string pre = "block" + std::to_string(k + 1) + ".";
        HedBlock& b = t.blk[k];
        b.convs.clear();
        for (int j = 0; j < kLayers[k]; ++j) {
            const std::string name = pre + "convs." + std::to_string(j);
            if (k == 0 && j == 0) {
                TRY(ps.conv_direct(name, kC[0], 3, &t.stem));
            } else {
                b.convs.emplace_back();
                TRY(ps.conv(name, kC[k], cin, 3, false, &b.convs.back()));
            }
            cin = kC[k];
        }
        TRY(ps.raw_f32(pre + "projection.weight", {1, kC[k], 1, 1}, &b.pw));
        TRY(ps.raw_f32(pre + "projection.bias", {1}, &b.pb));
    }
    return 0;
}

// after packing: norm to the host (a kernel argument of the stem), the biases of the trunk multiplied by the scale, the range flag
int finish_build(Hed& t, hipStream_t s) {
    const float sc = t.cfg.trunk_scale;
    if (sc != 1.f) {
        TRY(op_hed_scale_vec(t.stem.b, kC[0], sc, s));
        for (int k = 0; k < kBlocks; ++k)
            for (const ConvW& c : t.blk[k].convs) TRY(op_hed_scale_vec(c.b, c.Cout, sc, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(t.norm_host, t.norm, 3 * sizeof(float), hipMemcpyDeviceToHost));
    TRY(t.pk->dalloc(256, (void**)&t.flag));
    HIP_TRY(hipMemset(t.flag, 0, 256));
    return 0;
}

struct HedFwd {
    const unsigned char* src; int N, H, W, scribble, ch;
    unsigned char* out; float* logits;
};

// frames [f0, f0 + n) of the call
int run_group(Ctx& cx, const Hed& t, const HedFwd& a, int f0, int n) {
    const size_t HW = (size_t)a.H * a.W;
    const float sc = t.cfg.trunk_scale;
    half_t* x = cx.h((size_t)n * HW * kC[0]);
    half_t* y = cx.h((size_t)n * HW * kC[0]);
    float* p[kBlocks];
    for (int k = 0; k < kBlocks; ++k) p[k] = cx.f((size_t)n * (HW >> (2 * k)));
    RUN(cx, op_hed_stem(a.src + (size_t)f0 * HW * 3, n, a.H, a.W, t.stem.w, t.stem.b, t.norm_host, sc, x, t.flag, cx.s));
    int h = a.H, w = a.W;
    for (int k = 0; k < kBlocks; ++k) {
        for (const ConvW& c : t.blk[k].convs) {
            IGemmArgs g = {};
            g.A = x; g.lda = c.Cin; g.mode = IG_CONV2D; g.Cin = c.Cin; g.taps = 9;
            g.Hin = h; g.Win = w; g.Hout = h; g.Wout = w; g.stride = 1; g.up = 1;
            g.W = c.w; g.M = n * h * w; g.Nout = c.Cout; g.Ktot = 9 * c.Cin;
            g.bias = c.b; g.rows_per_img = h * w; g.scale = 1.f; g.act = 3;
            g.nseg = 1;
            g.seg[0] = IGemmSeg{y, c.Cout, 0, c.Cout, SEG_ROW, DT_F16, 1, 0};
            g.nonfinite = t.flag;
            RUN(cx, op_igemm(g, cx.s));
            std::swap(x, y);
        }
        const bool pool = k + 1 < kBlocks;
        RUN(cx, op_hed_pool_proj(x, n, h, w, kC[k], t.blk[k].pw, t.blk[k].pb, 1.f / sc, pool ? y : nullptr, p[k], cx.s));
        if (pool) { std::swap(x, y); h /= 2; w /= 2; }
    }
    float* lg = a.logits ? a.logits + (size_t)f0 * HW : nullptr;
    if (!a.scribble) {
        RUN(cx, op_hed_fuse(p, n, a.H, a.W, a.ch, a.out + (size_t)f0 * HW * a.ch, lg, cx.s));
        return 0;
    }
    unsigned char* soft = (unsigned char*)cx.alloc((size_t)n * HW);
    float* blurred = cx.f((size_t)n * HW);
    unsigned char* thin = (unsigned char*)cx.alloc((size_t)n * HW);
    RUN(cx, op_hed_fuse(p, n, a.H, a.W, 1, soft, lg, cx.s));
    RUN(cx, op_hed_blur_f32(soft, n, a.H, a.W, blurred, cx.s));
    RUN(cx, op_hed_nms(blurred, n, a.H, a.W, thin, cx.s));
    RUN(cx, op_hed_blur_u8_bin(thin, n, a.H, a.W, a.ch, a.out + (size_t)f0 * HW * a.ch, cx.s));
    return 0;
}

int check_args(const HedFwd& a, int fpg) {
    CTRL_CHECK(a.N >= 1, "hed: at least one frame is required");
    CTRL_CHECK(a.H >= 64 && a.W >= 64 && a.H % 64 == 0 && a.W % 64 == 0 && a.H <= 4096 && a.W <= 4096,
               "hed: H and W must be multiples of 64 (what HEDdetector's resize_image produces), at most 4096");
    CTRL_CHECK(a.ch == 1 || a.ch == 3, "hed: out_channels must be 1 or 3");
    CTRL_CHECK(fpg >= 0, "hed: frames_per_group must be 0 (sized from the workspace cap) or positive");
    return 0;
}

size_t dry_bytes(const Hed& t, const HedFwd& a, int n) {
    Arena tmp;
    Ctx dry{&tmp, nullptr, true};
    (void)run_group(dry, t, a, 0, n);
    return tmp.peak + 1024;
}

// frames per group: the caller's, or equal groups of the largest size below the cap; always within the 2^31-element index rule of the
// launches (n * H * W * 64 elements in the widest map)
int group_size(const Hed& t, const HedFwd& a, int fpg) {
    const double lim = std::floor((2147483648.0 - 1.0) / ((double)a.H * a.W * kC[0]));
    const int idx_max = (int)std::min(lim, 4096.0);
    if (idx_max < 1) return 0;
    if (fpg > 0) return std::min(std::min(fpg, a.N), idx_max);
    const size_t cap = t.cfg.ws_cap_bytes > 0 ? (size_t)t.cfg.ws_cap_bytes : kDefaultCap;
    const size_t one = dry_bytes(t, a, 1);
    const int gmax = (int)std::max<size_t>(1, std::min<size_t>(cap / one, (size_t)idx_max));
    const int groups = (a.N + gmax - 1) / gmax;
    return (a.N + groups - 1) / groups;
}

int forward(Hed& t, const HedFwd& a, int fpg, hipStream_t s) {
    CTRL_CHECK(a.src != nullptr && a.out != nullptr, "hed: frames and out are required");
    TRY(check_args(a, fpg));
    CTRL_CHECK(((uintptr_t)a.out & 3) == 0, "hed: out must be 4-byte aligned");
    const int g = group_size(t, a, fpg);
    CTRL_CHECK(g >= 1, "hed: the frame is too large for one launch");
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    CTRL_CHECK(!capturing, "hed: the stream is capturing; the forward reads its fp16 range flag back at the end and cannot be recorded "
                           "into a graph");
    TRY(t.reserve(dry_bytes(t, a, g), false, "hed", "group of frames"));
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
    CTRL_CHECK(bad == 0, "hed: an activation left the fp16 range (|x| > 65504) -- the output is not valid; create the detector with a "
                         "smaller trunk_scale (a power of two below " + std::to_string(t.cfg.trunk_scale) + ")");
    return 0;
}

}  // namespace

extern "C" {

int ctrl_hed_create(const ctrl_hed_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_hed** out) {
    return plan_create<Hed>("hed_create", cfg, tensors, n_tensors, stream, (void**)out, validate, build_hed, finish_build);
}

void ctrl_hed_destroy(ctrl_hed* h) { plan_destroy<Hed>(h); }

int ctrl_hed_forward(ctrl_hed* h, const void* frames_u8, int N, int H, int W, int scribble, int out_channels, void* out_u8, float* logits,
                     int frames_per_group, void* stream) {
    CTRL_CHECK(h != nullptr, "hed_forward: null plan");
    Hed* t = (Hed*)h;
    DeviceGuard dg(t->device);
    const HedFwd a = {(const unsigned char*)frames_u8, N, H, W, scribble ? 1 : 0, out_channels, (unsigned char*)out_u8, logits};
    return forward(*t, a, frames_per_group, S(stream));
}

int64_t ctrl_hed_ws_bytes(ctrl_hed* h, int N, int H, int W, int scribble, int frames_per_group) {
    if (!h) return 0;
    const Hed* t = (const Hed*)h;
    const HedFwd a = {nullptr, N, H, W, scribble ? 1 : 0, 3, nullptr, nullptr};
    if (check_args(a, frames_per_group)) return 0;
    const int g = group_size(*t, a, frames_per_group);
    return g >= 1 ? (int64_t)dry_bytes(*t, a, g) : 0;
}

int ctrl_op_hed_stem(const void* src_u8, int N, int H, int W, const float* w, const float* bias, const float* norm_host3, float scale,
                     void* out_f16, int32_t* nonfinite, void* stream) {
    return op_hed_stem((const unsigned char*)src_u8, N, H, W, w, bias, norm_host3, scale, (half_t*)out_f16, nonfinite, S(stream));
}
int ctrl_op_hed_pool_proj(const void* h_f16, int N, int H, int W, int C, const float* wp, const float* bp, float inv_scale, void* pooled_f16,
                          float* p, void* stream) {
    return op_hed_pool_proj((const half_t*)h_f16, N, H, W, C, wp, bp, inv_scale, (half_t*)pooled_f16, p, S(stream));
}
int ctrl_op_hed_fuse(const float* const* maps, int N, int H, int W, int out_channels, void* out_u8, float* logits, void* stream) {
    return op_hed_fuse(maps, N, H, W, out_channels, (unsigned char*)out_u8, logits, S(stream));
}
int ctrl_op_hed_blur_f32(const void* src_u8, int N, int H, int W, float* out, void* stream) {
    return op_hed_blur_f32((const unsigned char*)src_u8, N, H, W, out, S(stream));
}
int ctrl_op_hed_nms(const float* x, int N, int H, int W, void* out_u8, void* stream) {
    return op_hed_nms(x, N, H, W, (unsigned char*)out_u8, S(stream));
}
int ctrl_op_hed_blur_u8_bin(const void* src_u8, int N, int H, int W, int out_channels, void* out_u8, void* stream) {
    return op_hed_blur_u8_bin((const unsigned char*)src_u8, N, H, W, out_channels, (unsigned char*)out_u8, S(stream));
}

}  // extern "C"
