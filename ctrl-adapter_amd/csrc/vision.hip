// CLIP vision tower kernels (transformers CLIPVisionModelWithProjection: the image_encoder of SVD and I2VGen-XL, CLIP ViT-H/14;
// svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212 and i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:366-396):
//   vision_patchify_kernel  pixels -> im2col rows [N*P][Kpad] fp16 of the patch convolution (kernel = stride = patch), optionally
//                           normalised (x - mean_c) / std_c in fp32 first (uint8 read as x / 255): one rounding, as torch's "normalise, then .to(fp16)"
//   vision_embed_ln_kernel  [class ; patch GEMM rows] + position -> pre_layrnorm (the fp32 residual stream) -> layer 0's layer_norm1 (fp16)
//   vision_vt_kernel        V of the row-major Q | K | V GEMM output -> V^T [N][C][Lkpad] for the flash attention, pad columns zeroed
//   vision_cls_ln_kernel    post_layernorm of row 0 of every image (the pooled output, + an fp32 copy for the projection)
//   clip_resize_aa_kernel   SVD's _resize_with_antialiasing (Gaussian blur, reflect padding, bicubic align_corners) + CLIP normalise
// Every kernel computes a row, an image's tile or a pixel on its own: an image's results do not depend on the batch it is in.
#include "ops.h"
#include <math.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int kRowThreads = 256;
constexpr int kRowPer = 8;           // C <= 2048

// sum over the 256 threads of a row workgroup (4 waves), same value in every thread (the row kernels of text.hip)
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// LayerNorm of the kRowPer values a thread holds (columns threadIdx.x + i * 256 < C), two-pass statistics in fp32
__device__ __forceinline__ void row_ln(float (&v)[kRowPer], int C, float eps, const float* g, const float* b, float* red) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) s += v[i];
    const float mean = block_sum256(s, red) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        const float d = c < C ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum256(q, red) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) v[i] = (v[i] - mean) * rstd * g[c] + b[c];
    }
}

struct PixNorm {
    int on;
    float mean[3], std[3];
};

__device__ __forceinline__ float load_pixel(const void* px, int dt, int n, int c, int y, int x, int H, int W) {
    if (dt == CTRL_U8_NHWC)           // pil_to_numpy: float32(x) / 255 (a correctly rounded fp32 division)
        return (float)((const unsigned char*)px)[(((size_t)n * H + y) * W + x) * 3 + c] / 255.0f;
    return load_as_f32(px, (((size_t)n * 3 + c) * H + y) * W + x, dt);
}

// one thread per output element: row m = (image n, patch py * G + px), column k = c * p * p + ky * p + kx (the conv weight's
// [Cout][3][p][p] order), zero for k >= 3 p p
__global__ __launch_bounds__(256) void vision_patchify_kernel(const void* __restrict__ px, int dt, int S, int p, int G, int Kpad, size_t total,
                                                              PixNorm nm, half_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % Kpad);
    const size_t m = i / Kpad;
    const int pp = p * p;
    float v = 0.f;
    if (k < 3 * pp) {
        const int P = G * G;
        const int n = (int)(m / P), q = (int)(m % P);
        const int c = k / pp, r = k - c * pp;
        const int y = (q / G) * p + r / p, x = (q % G) * p + r % p;
        v = load_pixel(px, dt, n, c, y, x, S, S);
        if (nm.on) v = (v - nm.mean[c]) / nm.std[c];
    }
    out[i] = (half_t)v;
}

// one workgroup per token row (image n, token r): e = (r == 0 ? class : patch_out[n * (L - 1) + r - 1]) + pos[r];
// x = pre_layrnorm(e) (fp32 stream), y = layer_norm1(x) (fp16 operand of the first Q | K | V GEMM)
__global__ __launch_bounds__(kRowThreads) void vision_embed_ln_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                                      const float* __restrict__ pos, int L, int C,
                                                                      const float* __restrict__ g0, const float* __restrict__ b0,
                                                                      const float* __restrict__ g1, const float* __restrict__ b1, float eps,
                                                                      float* __restrict__ x, half_t* __restrict__ y) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    const int n = row / L, r = row - n * L;
    const float* src = r == 0 ? cls : patch + ((size_t)n * (L - 1) + r - 1) * C;
    const float* pe = pos + (size_t)r * C;
    float v[kRowPer];
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        v[i] = c < C ? src[c] + pe[c] : 0.f;
    }
    row_ln(v, C, eps, g0, b0, red);
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) x[(size_t)row * C + c] = v[i];
    }
    row_ln(v, C, eps, g1, b1, red);
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) y[(size_t)row * C + c] = (half_t)v[i];
    }
}

// 32 x 32 tile of one image: vt[n][c][l] = v[n * L + l][c] for l < L, 0 for L <= l < Lkpad (the attention reads finite pad columns)
__global__ __launch_bounds__(256) void vision_vt_kernel(const half_t* __restrict__ v, long ld, half_t* __restrict__ vt, int L, int C, int Lkpad) {
    __shared__ half_t tile[32][33];
    const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32, n = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int l = l0 + j;
        tile[j][tx] = l < L ? v[((size_t)n * L + l) * ld + c0 + tx] : (half_t)0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) vt[((size_t)n * C + c0 + j) * Lkpad + l0 + tx] = tile[tx][j];
}

// one workgroup per image: LayerNorm of row 0 (x + n * L * C) into pooled [N][C] (y_dt) and pooled32 [N][C] fp32 (either may be null)
__global__ __launch_bounds__(kRowThreads) void vision_cls_ln_kernel(const float* __restrict__ x, int L, int C, const float* __restrict__ g,
                                                                    const float* __restrict__ b, float eps, void* __restrict__ pooled, int y_dt,
                                                                    float* __restrict__ pooled32) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const float* xr = x + (size_t)n * L * C;
    float v[kRowPer];
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        v[i] = c < C ? xr[c] : 0.f;
    }
    row_ln(v, C, eps, g, b, red);
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) {
            if (pooled) store_from_f32(pooled, (size_t)n * C + c, y_dt, v[i]);
            if (pooled32) pooled32[(size_t)n * C + c] = v[i];
        }
    }
}

// ------------------------------------------------------------------------------------------ SVD's _resize_with_antialiasing
constexpr int kMaxTaps = 63;

struct ResizeArgs {
    const void* src; int dt;               // fp32 / fp16 / bf16 NCHW in [0, 1], or uint8 NHWC (/ 255)
    int N, H, W, OH, OW;
    int ky, kx;                            // Gaussian taps (odd) along y / x
    float scale_y, scale_x;                // (in - 1) / (out - 1) in fp32 (align_corners)
    PixNorm nm;
    void* out; int out_dt;                 // [N][3][OH][OW]
    float wy[kMaxTaps], wx[kMaxTaps];      // normalised Gaussian taps, computed as torch does in fp32
};

__device__ __forceinline__ int reflect(int i, int n) {      // torch "reflect" padding (the edge is not repeated); pad < n
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// A = -0.75 cubic convolution weights of torch's upsample_bicubic2d
__device__ __forceinline__ void cubic_w(float t, float (&w)[4]) {
    const float A = -0.75f;
    auto c1 = [A](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
    auto c2 = [A](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
    w[0] = c2(t + 1.f);
    w[1] = c1(t);
    w[2] = c1(1.f - t);
    w[3] = c2(2.f - t);
}

// the blurred pixel (c, y, x) of image n in the reference's order: the x pass (on x * 2 - 1), then the y pass
__device__ __forceinline__ float blurred(const ResizeArgs& a, int n, int c, int y, int x) {
    const int py = a.ky >> 1, pxh = a.kx >> 1;
    float acc = 0.f;
    for (int ty = 0; ty < a.ky; ++ty) {
        const int yy = reflect(y + ty - py, a.H);
        float row = 0.f;
        for (int tx = 0; tx < a.kx; ++tx) {
            const int xx = reflect(x + tx - pxh, a.W);
            row += a.wx[tx] * (load_pixel(a.src, a.dt, n, c, yy, xx, a.H, a.W) * 2.f - 1.f);
        }
        acc += a.wy[ty] * row;
    }
    return acc;
}

__global__ __launch_bounds__(256) void clip_resize_aa_kernel(ResizeArgs a) {
    const size_t total = (size_t)a.N * 3 * a.OH * a.OW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % a.OW);
    const int oy = (int)((i / a.OW) % a.OH);
    const int c = (int)((i / ((size_t)a.OW * a.OH)) % 3);
    const int n = (int)(i / ((size_t)a.OW * a.OH * 3));
    // torch: real = scale * dst; in = min(floor(real), in - 1); t = clamp(real - in, 0, 1); taps in - 1 .. in + 2 clamped to the image
    const float ry = a.scale_y * (float)oy, rx = a.scale_x * (float)ox;
    const int iy = min((int)floorf(ry), a.H - 1), ix = min((int)floorf(rx), a.W - 1);
    const float ty = fminf(fmaxf(ry - (float)iy, 0.f), 1.f), tx = fminf(fmaxf(rx - (float)ix, 0.f), 1.f);
    float wy[4], wx[4];
    cubic_w(ty, wy);
    cubic_w(tx, wx);
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = min(max(iy - 1 + j, 0), a.H - 1);
        float r = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) r += wx[k] * blurred(a, n, c, y, min(max(ix - 1 + k, 0), a.W - 1));
        v += wy[j] * r;
    }
    v = (v + 1.f) / 2.f;
    if (a.nm.on) v = (v - a.nm.mean[c]) / a.nm.std[c];
    store_from_f32(a.out, i, a.out_dt, v);
}

// the reference's sigma and kernel size along one axis (skimage's rule, 2 sigma each side, odd, at least 3) and its fp32 taps
int gauss_taps(int in, int out, float* w, int* ks) {
    const double sigma = std::max(((double)in / out - 1.0) / 2.0, 0.001);
    int k = (int)std::max(2.0 * 2 * sigma, 3.0);
    if (k % 2 == 0) k += 1;
    CTRL_CHECK(k <= kMaxTaps, "clip_resize_aa: the down-sampling factor is too large (Gaussian of more than 63 taps)");
    CTRL_CHECK(k / 2 < in, "clip_resize_aa: the image is smaller than the blur's reflect padding");
    const float s = (float)sigma;
    const float den = 2.f * (s * s);
    float sum = 0.f;
    for (int i = 0; i < k; ++i) {
        const float x = (float)(i - k / 2);
        w[i] = std::exp(-(x * x) / den);
        sum += w[i];
    }
    for (int i = 0; i < k; ++i) w[i] = w[i] / sum;
    *ks = k;
    return 0;
}

PixNorm make_norm(const float* mean_std) {
    PixNorm nm = {};
    if (mean_std) {
        nm.on = 1;
        for (int c = 0; c < 3; ++c) { nm.mean[c] = mean_std[c]; nm.std[c] = mean_std[3 + c]; }
    }
    return nm;
}

// fp32 conv weight [C][3][p][p] -> fp16 [C][Kpad] (columns >= 3 p p zero): the patch GEMM's B operand
__global__ void vision_pack_patch_kernel(const float* __restrict__ w, int K, int Kpad, size_t total, half_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % Kpad);
    out[i] = k < K ? (half_t)w[(i / Kpad) * K + k] : (half_t)0.f;
}

}  // namespace

int op_vision_patchify(const void* px, int dt, int N, int S, int p, const float* mean_std, half_t* out, int Kpad, hipStream_t s) {
    CTRL_CHECK(px && out, "vision_patchify: null argument");
    CTRL_CHECK(dt == DT_F32 || dt == DT_F16 || dt == DT_BF16 || dt == CTRL_U8_NHWC, "vision_patchify: pixel dtype must be fp32, fp16, bf16 or uint8 NHWC");
    CTRL_CHECK(N >= 1 && p >= 1 && S >= p && S % p == 0, "vision_patchify: image_size must be a positive multiple of patch_size");
    CTRL_CHECK(Kpad >= 3 * p * p && Kpad % 64 == 0, "vision_patchify: Kpad must be a multiple of 64 >= 3 * patch_size^2");
    for (int c = 0; mean_std && c < 3; ++c) CTRL_CHECK(mean_std[3 + c] != 0.f, "vision_patchify: std must be non-zero");
    const int G = S / p;
    const size_t total = (size_t)N * G * G * Kpad;
    PROF_WORK(0, (double)N * 3 * S * S * (dt == DT_F32 ? 4 : dt == CTRL_U8_NHWC ? 1 : 2) + (double)total * 2);
    LAUNCH("vision_patchify", vision_patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, px, dt, S, p, G, Kpad, total,
           make_norm(mean_std), out);
    return 0;
}

int op_vision_embed(const float* patch, const float* cls, const float* pos, int N, int L, int C, const float* g0, const float* b0,
                    const float* g1, const float* b1, float eps, float* x, half_t* y, hipStream_t s) {
    CTRL_CHECK(patch && cls && pos && g0 && b0 && g1 && b1 && x && y, "vision_embed: null argument");
    CTRL_CHECK(N >= 1 && L >= 2 && C >= 1 && C <= kRowThreads * kRowPer, "vision_embed: bad shape (L >= 2, C <= 2048)");
    PROF_WORK(0, (double)N * L * C * (4.0 * 2 + 4.0 + 2.0));
    LAUNCH("vision_embed", vision_embed_ln_kernel, dim3(N * L), dim3(kRowThreads), 0, s, patch, cls, pos, L, C, g0, b0, g1, b1, eps, x, y);
    return 0;
}

int op_vision_vt(const half_t* v, long ld, half_t* vt, int N, int L, int C, int Lkpad, hipStream_t s) {
    CTRL_CHECK(v && vt, "vision_vt: null argument");
    CTRL_CHECK(N >= 1 && L >= 1 && C % 32 == 0 && Lkpad % 32 == 0 && Lkpad >= L && ld >= C, "vision_vt: bad shape");
    PROF_WORK(0, (double)N * C * (L + Lkpad) * 2.0);
    LAUNCH("vision_vt", vision_vt_kernel, dim3(Lkpad / 32, C / 32, N), dim3(256), 0, s, v, ld, vt, L, C, Lkpad);
    return 0;
}

int op_vision_cls_ln(const float* x, int N, int L, int C, const float* g, const float* b, float eps, void* pooled, int y_dt, float* pooled32,
                     hipStream_t s) {
    CTRL_CHECK(x && g && b && (pooled || pooled32), "vision_cls_ln: null argument");
    CTRL_CHECK(N >= 1 && L >= 1 && C >= 1 && C <= kRowThreads * kRowPer, "vision_cls_ln: bad shape (C <= 2048)");
    CTRL_CHECK(y_dt >= DT_F32 && y_dt <= DT_BF16, "vision_cls_ln: bad dtype");
    PROF_WORK(0, (double)N * C * 10.0);
    LAUNCH("vision_cls_ln", vision_cls_ln_kernel, dim3(N), dim3(kRowThreads), 0, s, x, L, C, g, b, eps, pooled, y_dt, pooled32);
    return 0;
}

int op_clip_resize_aa(const void* src, int dt, int N, int H, int W, int OH, int OW, const float* mean_std, void* out, int out_dt, hipStream_t s) {
    CTRL_CHECK(src && out, "clip_resize_aa: null argument");
    CTRL_CHECK(dt == DT_F32 || dt == DT_F16 || dt == DT_BF16 || dt == CTRL_U8_NHWC, "clip_resize_aa: input dtype must be fp32, fp16, bf16 or uint8 NHWC");
    CTRL_CHECK(out_dt == DT_F32 || out_dt == DT_F16 || out_dt == DT_BF16, "clip_resize_aa: out_dtype must be fp32, fp16 or bf16");
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1 && OH >= 2 && OW >= 2, "clip_resize_aa: bad shape (output at least 2 x 2)");
    CTRL_CHECK((size_t)N * 3 * OH * OW < (1ull << 31) * 256ull, "clip_resize_aa: output too large");
    for (int c = 0; mean_std && c < 3; ++c) CTRL_CHECK(mean_std[3 + c] != 0.f, "clip_resize_aa: std must be non-zero");
    ResizeArgs a = {};
    a.src = src; a.dt = dt; a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    TRY(gauss_taps(H, OH, a.wy, &a.ky));
    TRY(gauss_taps(W, OW, a.wx, &a.kx));
    a.scale_y = (float)(H - 1) / (float)(OH - 1);
    a.scale_x = (float)(W - 1) / (float)(OW - 1);
    a.nm = make_norm(mean_std);
    a.out = out; a.out_dt = out_dt;
    const size_t total = (size_t)N * 3 * OH * OW;
    PROF_WORK(2.0 * total * 16 * a.ky * (a.kx + 1), (double)N * 3 * H * W * (dt == DT_F32 ? 4 : dt == CTRL_U8_NHWC ? 1 : 2) +
                                                    (double)total * (out_dt == DT_F32 ? 4 : 2));
    LAUNCH("clip_resize_aa", clip_resize_aa_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return 0;
}

int op_vision_pack_patch(const float* w, int C, int K, int Kpad, half_t* out, hipStream_t s) {
    CTRL_CHECK(w && out && C >= 1 && K >= 1 && Kpad >= K, "vision_pack_patch: bad argument");
    const size_t total = (size_t)C * Kpad;
    LAUNCH("vision_pack_patch", vision_pack_patch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, K, Kpad, total, out);
    return 0;
}
