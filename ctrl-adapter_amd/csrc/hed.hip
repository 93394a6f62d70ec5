// HED annotator (controlnet_aux ControlNetHED_Apache2 + HEDdetector: the reference's `scribble` condition, model/ctrl_helper.py:124-127,
// 196-197, and ControlNet's soft-edge condition).  The memory-bound kernels around the VGG trunk, whose other twelve 3x3 convolutions
// run on the implicit GEMM with act = 3 (ReLU).  Activations fp16 NHWC, accumulation fp32.
//   stem       uint8 frame -> (x - norm) * s -> conv1_1 (3 -> 64, K = 27) + bias + ReLU -> fp16 NHWC, one launch
//   pool+proj  reads a block's output h once: the 2x2 max-pooled h of the next block and the block's 1x1 projection (fp32, one per pixel)
//   fuse       five projection maps -> cv2's INTER_LINEAR (half-pixel centres, float32, horizontal then vertical) -> mean -> sigmoid ->
//              * 255, clip, truncate -> uint8, 1 or 3 channels
//   tail       the scribble post-processing: separable Gaussian blur (25 taps to fp32, 19 taps to uint8 + binarise; reflect-101) and the
//              four-direction non-maximum suppression.  These three follow tests/hed_ref.py bit for bit: every tap is one rounded
//              multiply and one rounded add, left to right, rows before columns (mul_rn / add_rn below: nothing contracts to an fma).
#include "ops.h"
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr double kSigma = 3.0;               // HEDdetector: nms(x, 127, 3.0), GaussianBlur(x, (0, 0), 3.0)
constexpr int kTapsF32 = 25, kTapsU8 = 19;   // cv2's automatic ksize at sigma 3: round(sigma * 8 + 1) | 1 for float, round(sigma * 6 + 1) | 1 for uint8

// ---------------------------------------------------------------------------------------------------------------- stem
// one thread: four neighbouring pixels of a row x eight output channels; the 27 x 64 weights and the bias sit in LDS.
// grid: ceil(quads / 32) workgroups, quads = N * H * W / 4
__global__ __launch_bounds__(NT) void hed_stem_kernel(const unsigned char* __restrict__ src, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float n0, float n1, float n2, float scale, int H, int W,
                                                      long quads, half_t* __restrict__ out, int32_t* nonfinite) {
    __shared__ __attribute__((aligned(16))) float sw[27 * 64];
    __shared__ float sb[64];
    for (int i = threadIdx.x; i < 27 * 64; i += NT) sw[i] = w[i];
    if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int cg = threadIdx.x & 7;
    const long q = (long)blockIdx.x * (NT / 8) + (threadIdx.x >> 3);
    if (q >= quads) return;
    const int wq = W >> 2;
    const long row = q / wq;                       // n * H + y
    const int x0 = (int)(q - row * wq) * 4, y = (int)(row % H);
    const float nrm[3] = {n0, n1, n2};
    float in[3][6][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = y + dy - 1;
#pragma unroll
        for (int dx = 0; dx < 6; ++dx) {
            const int xx = x0 + dx - 1;
            const bool inb = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const unsigned char* p = src + ((row + (dy - 1)) * W + xx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) in[dy][dx][c] = inb ? ((float)p[c] - nrm[c]) * scale : 0.f;      // the padding is zero AFTER the subtraction
        }
    }
    float acc[4][8];
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[px][j] = sb[cg * 8 + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* wk = sw + ((ky * 3 + kx) * 3 + c) * 64 + cg * 8;
                const f4 w0 = *(const f4*)wk, w1 = *(const f4*)(wk + 4);
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    const float v = in[ky][px + kx][c];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[px][j] = fmaf(v, w0[j], acc[px][j]);
                        acc[px][4 + j] = fmaf(v, w1[j], acc[px][4 + j]);
                    }
                }
            }
    bool bad = false;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = acc[px][j] < 0.f ? 0.f : acc[px][j];
            bad = bad || !(v <= 65504.0f);
            o[j] = (half_t)v;
        }
        *(h8*)(out + ((size_t)row * W + x0 + px) * 64 + cg * 8) = o;
    }
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;          // (divergent code: any lane may raise the flag)
}

// ---------------------------------------------------------------------------------------------------------------- pool + project
// L = C / 8 lanes share one 2x2 block of pixels, eight channels each: four 16-byte loads, the channel-wise maximum stored as the pooled
// map (when given), the four dot products with the projection weights reduced over the L lanes in a fixed order
template <int L>
__global__ __launch_bounds__(NT) void hed_pool_proj_kernel(const half_t* __restrict__ h, const float* __restrict__ wp, const float* __restrict__ bp,
                                                           float inv_scale, int Hh, int Wh, long blocks2, half_t* __restrict__ pooled,
                                                           float* __restrict__ p) {
    constexpr int C = L * 8;
    const int l = threadIdx.x % L;
    const long q = (long)blockIdx.x * (NT / L) + threadIdx.x / L;
    if (q >= blocks2) return;                      // (whole groups of L lanes leave together: the shuffles below stay inside a group)
    const int hw2 = Hh * Wh, W = 2 * Wh;
    const long n = q / hw2;
    const int rem = (int)(q - n * hw2), y2 = rem / Wh, x2 = rem - y2 * Wh;
    const size_t pix = ((size_t)n * 2 * Hh + 2 * y2) * W + 2 * x2;
    const half_t* b = h + pix * C + l * 8;
    const h8 v[4] = {*(const h8*)b, *(const h8*)(b + C), *(const h8*)(b + (size_t)W * C), *(const h8*)(b + (size_t)W * C + C)};
    const f4 w0 = *(const f4*)(wp + l * 8), w1 = *(const f4*)(wp + l * 8 + 4);
    float s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v[i][j], w0[j], a);
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v[i][4 + j], w1[j], a);
#pragma unroll
        for (int o = L / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        s[i] = a;
    }
    if (l == 0) {
        const float bb = bp[0];
        p[pix] = fmaf(s[0], inv_scale, bb);
        p[pix + 1] = fmaf(s[1], inv_scale, bb);
        p[pix + W] = fmaf(s[2], inv_scale, bb);
        p[pix + W + 1] = fmaf(s[3], inv_scale, bb);
    }
    if (pooled) {
        h8 m;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const half_t a = v[0][j] > v[1][j] ? v[0][j] : v[1][j], c = v[2][j] > v[3][j] ? v[2][j] : v[3][j];
            m[j] = a > c ? a : c;
        }
        *(h8*)(pooled + (size_t)q * C + l * 8) = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- fuse
struct FuseMaps { const float* p[5]; };

// cv2.resize(INTER_LINEAR) of map k (stride 2^k) at output pixel (y, x): fx = (dx + 0.5) * scale - 0.5 in float, floor, both clamps,
// the row pair interpolated along x first, then along y
__device__ __forceinline__ void lin_coord(int d, float sc, int n, int* i0, int* i1, float* f) {
    float fx = ((float)d + 0.5f) * sc - 0.5f;
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= n - 1) { sx = n - 1; fx = 0.f; }
    *i0 = sx; *i1 = sx + 1 < n ? sx + 1 : n - 1; *f = fx;
}

template <int CH>
__global__ __launch_bounds__(NT) void hed_fuse_kernel(FuseMaps m, int H, int W, long quads, unsigned char* __restrict__ out,
                                                      float* __restrict__ logit) {
    const long q = (long)blockIdx.x * NT + threadIdx.x;
    if (q >= quads) return;
    const int wq = W >> 2;
    const long row = q / wq;
    const int x0 = (int)(q - row * wq) * 4, y = (int)(row % H);
    const long n = row / H;
    unsigned bytes = 0;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const int x = x0 + px;
        float sum = m.p[0][(size_t)row * W + x];
#pragma unroll
        for (int k = 1; k < 5; ++k) {
            const int hk = H >> k, wk = W >> k;
            const float sc = 1.0f / (float)(1 << k);
            int xa, xb, ya, yb;
            float fx, fy;
            lin_coord(x, sc, wk, &xa, &xb, &fx);
            lin_coord(y, sc, hk, &ya, &yb, &fy);
            const float* P = m.p[k] + (size_t)n * hk * wk;
            const float r0 = P[ya * wk + xa] * (1.f - fx) + P[ya * wk + xb] * fx;
            const float r1 = P[yb * wk + xa] * (1.f - fx) + P[yb * wk + xb] * fx;
            sum += r0 * (1.f - fy) + r1 * fy;
        }
        const float mean = sum / 5.0f;
        if (logit) logit[(size_t)row * W + x] = mean;
        float u = (1.0f / (1.0f + expf(-mean))) * 255.0f;
        u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
        bytes |= (unsigned)(unsigned char)u << (8 * px);          // astype(uint8): truncation
    }
    if (CH == 1) {
        *(unsigned*)(out + (size_t)row * W + x0) = bytes;
    } else {
        const unsigned b0 = bytes & 255u, b1 = (bytes >> 8) & 255u, b2 = (bytes >> 16) & 255u, b3 = bytes >> 24;
        unsigned* o = (unsigned*)(out + ((size_t)row * W + x0) * 3);
        o[0] = b0 | (b0 << 8) | (b0 << 16) | (b1 << 24);
        o[1] = b1 | (b1 << 8) | (b2 << 16) | (b2 << 24);
        o[2] = b2 | (b3 << 8) | (b3 << 16) | (b3 << 24);
    }
}

// ---------------------------------------------------------------------------------------------------------------- scribble tail
struct Taps { float v[kTapsF32]; };

// One rounded multiply, one rounded add.  hipcc contracts a * b + c into an fma by default, and HIP's own __fmul_rn / __fadd_rn are inline
// functions compiled under that default (their * and + fuse again once inlined): from here to the end of the file nothing contracts
// (explicit fmaf calls are not affected), and the two helpers are defined under that rule.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);       // (only positions outside a partial tile's image part ever need the clamp)
}

// separable KS-tap blur of a uint8 map over a 64 x 64 tile: the tile with its halo in LDS (bytes), the row pass over the tile's and the
// halo's rows into LDS (fp32), the column pass from there.  BIN: cv2's uint8 result (round half to even, saturate) and HED's binarise
// (> 4 -> 255, else 0) into CH channels; else the fp32 result.
template <int KS, bool BIN>
__global__ __launch_bounds__(NT) void hed_blur_kernel(const unsigned char* __restrict__ src, int H, int W, int tx, int ty, Taps k,
                                                      float* __restrict__ outf, unsigned char* __restrict__ outb, int CH) {
    constexpr int R = KS / 2, TS = 64, SW = TS + 2 * R, SP = (SW + 3) & ~3;
    __shared__ unsigned char s[SW][SP];
    __shared__ float t[SW][TS];
    const int tile = blockIdx.x, n = tile / (tx * ty), tr = tile - n * tx * ty, y0 = (tr / tx) * TS, x0 = (tr % tx) * TS;
    const unsigned char* img = src + (size_t)n * H * W;
    for (int i = threadIdx.x; i < SW * SW; i += NT) {
        const int ly = i / SW, lx = i - ly * SW;
        s[ly][lx] = img[(size_t)reflect101(y0 + ly - R, H) * W + reflect101(x0 + lx - R, W)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SW * TS; i += NT) {
        const int ly = i / TS, lx = i - ly * TS;
        float acc = mul_rn((float)s[ly][lx], k.v[0]);
#pragma unroll
        for (int j = 1; j < KS; ++j) acc = add_rn(acc, mul_rn((float)s[ly][lx + j], k.v[j]));
        t[ly][lx] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TS * TS; i += NT) {
        const int ly = i / TS, lx = i - ly * TS, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float acc = mul_rn(t[ly][lx], k.v[0]);
#pragma unroll
        for (int j = 1; j < KS; ++j) acc = add_rn(acc, mul_rn(t[ly + j][lx], k.v[j]));
        const size_t o = ((size_t)n * H + gy) * W + gx;
        if (BIN) {
            float r = rintf(acc);
            r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
            const unsigned char b = r > 4.f ? 255 : 0;
            for (int c = 0; c < CH; ++c) outb[o * CH + c] = b;
        } else {
            outf[o] = acc;
        }
    }
}

// controlnet_aux nms(x, t, s) behind its blur: keep a pixel that cv2.dilate leaves unchanged under one of the four 3-pixel line kernels
// (it is >= both neighbours on that line; neighbours outside the image do not count), 255 where a kept value is > thr
__global__ __launch_bounds__(NT) void hed_nms_kernel(const float* __restrict__ x, int H, int W, size_t total, float thr,
                                                     unsigned char* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int px = (int)(i % W), py = (int)((i / W) % H);
    const float* img = x + (i - (size_t)py * W - px);
    const float v = img[(size_t)py * W + px];
    const int dxs[4] = {1, 0, 1, 1}, dys[4] = {0, 1, 1, -1};
    bool keep = false;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int ax = px - dxs[d], ay = py - dys[d], bx = px + dxs[d], by = py + dys[d];
        const bool ain = ax >= 0 && ax < W && ay >= 0 && ay < H, bin = bx >= 0 && bx < W && by >= 0 && by < H;
        const float a = ain ? img[(size_t)ay * W + ax] : -INFINITY, b = bin ? img[(size_t)by * W + bx] : -INFINITY;
        keep = keep || (v >= a && v >= b);
    }
    out[i] = (keep && v > thr) ? 255 : 0;
}

__global__ void hed_scale_vec_kernel(float* v, int n, float s) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) v[i] *= s;
}

// cv2.getGaussianKernel(n, sigma) as the restatement takes it: exp in double, normalised in double, cast to float
Taps gaussian_taps(int n) {
    Taps t = {};
    double e[kTapsF32], sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = (double)i - (double)(n - 1) * 0.5;
        e[i] = std::exp(-(x * x) / (2.0 * kSigma * kSigma));
        sum += e[i];
    }
    for (int i = 0; i < n; ++i) t.v[i] = (float)(e[i] / sum);
    return t;
}

int check_map(const char* what, int N, int H, int W, int per_pixel) {
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1, std::string(what) + ": N, H and W must be positive");
    CTRL_CHECK((double)N * H * W * per_pixel < 2147483648.0, std::string(what) + ": the batch must stay below 2^31 elements; split it");
    return 0;
}

}  // namespace

int op_hed_stem(const unsigned char* src, int N, int H, int W, const float* w, const float* bias, const float* norm3, float scale, half_t* out,
                int32_t* nonfinite, hipStream_t s) {
    CTRL_CHECK(src && w && bias && norm3 && out, "hed_stem: null pointer");
    TRY(check_map("hed_stem", N, H, W, 64));
    CTRL_CHECK(W % 4 == 0, "hed_stem: W must be a multiple of 4");
    CTRL_CHECK(scale > 0.f, "hed_stem: the scale must be positive");
    const long quads = (long)N * H * W / 4;
    PROF_WORK(2.0 * 27 * 64 * N * H * W, (double)N * H * W * (3 + 128));
    LAUNCH("hed", hed_stem_kernel, dim3((unsigned)((quads + NT / 8 - 1) / (NT / 8))), dim3(NT), 0, s, src, w, bias, norm3[0], norm3[1], norm3[2],
           scale, H, W, quads, out, nonfinite);
    return 0;
}

int op_hed_pool_proj(const half_t* h, int N, int H, int W, int C, const float* wp, const float* bp, float inv_scale, half_t* pooled, float* p,
                     hipStream_t s) {
    CTRL_CHECK(h && wp && bp && p, "hed_pool_proj: null pointer");
    TRY(check_map("hed_pool_proj", N, H, W, C));
    CTRL_CHECK(H % 2 == 0 && W % 2 == 0, "hed_pool_proj: H and W must be even");
    CTRL_CHECK(C == 64 || C == 128 || C == 256 || C == 512, "hed_pool_proj: C must be 64, 128, 256 or 512");
    const int Hh = H / 2, Wh = W / 2, L = C / 8;
    const long blocks2 = (long)N * Hh * Wh;
    const dim3 grid((unsigned)((blocks2 + NT / L - 1) / (NT / L)));
    PROF_WORK(2.0 * C * N * H * W, (double)N * H * W * (2.0 * C * (pooled ? 1.25 : 1.0) + 4));
#define HED_PP(LL) LAUNCH("hed", hed_pool_proj_kernel<LL>, grid, dim3(NT), 0, s, h, wp, bp, inv_scale, Hh, Wh, blocks2, pooled, p)
    if (L == 8) HED_PP(8);
    else if (L == 16) HED_PP(16);
    else if (L == 32) HED_PP(32);
    else HED_PP(64);
#undef HED_PP
    return 0;
}

int op_hed_fuse(const float* const* maps5, int N, int H, int W, int out_channels, unsigned char* out, float* logits, hipStream_t s) {
    CTRL_CHECK(maps5 && out, "hed_fuse: null pointer");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "hed_fuse: out_channels must be 1 or 3");
    TRY(check_map("hed_fuse", N, H, W, 3));
    CTRL_CHECK(H % 16 == 0 && W % 16 == 0, "hed_fuse: H and W must be multiples of 16 (the five maps have strides 1 .. 16)");
    CTRL_CHECK(((uintptr_t)out & 3) == 0, "hed_fuse: out must be 4-byte aligned");
    FuseMaps m;
    for (int k = 0; k < 5; ++k) {
        CTRL_CHECK(maps5[k] != nullptr, "hed_fuse: null map");
        m.p[k] = maps5[k];
    }
    const long quads = (long)N * H * W / 4;
    const dim3 grid((unsigned)((quads + NT - 1) / NT));
    PROF_WORK(0, (double)N * H * W * (4.0 * 1.34 + out_channels + (logits ? 4 : 0)));
    if (out_channels == 3) LAUNCH("hed", hed_fuse_kernel<3>, grid, dim3(NT), 0, s, m, H, W, quads, out, logits);
    else LAUNCH("hed", hed_fuse_kernel<1>, grid, dim3(NT), 0, s, m, H, W, quads, out, logits);
    return 0;
}

static int blur_dims(const char* what, int N, int H, int W, int taps, long* tiles, int* tx, int* ty) {
    TRY(check_map(what, N, H, W, 4));
    CTRL_CHECK(H > taps / 2 && W > taps / 2, std::string(what) + ": H and W must exceed the blur radius (one reflection at a border)");
    *tx = (W + 63) / 64; *ty = (H + 63) / 64;
    *tiles = (long)N * *tx * *ty;
    return 0;
}

int op_hed_blur_f32(const unsigned char* src, int N, int H, int W, float* out, hipStream_t s) {
    CTRL_CHECK(src && out, "hed_blur_f32: null pointer");
    long tiles; int tx, ty;
    TRY(blur_dims("hed_blur_f32", N, H, W, kTapsF32, &tiles, &tx, &ty));
    PROF_WORK(4.0 * kTapsF32 * N * H * W, 5.0 * N * H * W);
    LAUNCH("hed", (hed_blur_kernel<kTapsF32, false>), dim3((unsigned)tiles), dim3(NT), 0, s, src, H, W, tx, ty, gaussian_taps(kTapsF32), out,
           (unsigned char*)nullptr, 1);
    return 0;
}

int op_hed_nms(const float* x, int N, int H, int W, unsigned char* out, hipStream_t s) {
    CTRL_CHECK(x && out, "hed_nms: null pointer");
    TRY(check_map("hed_nms", N, H, W, 4));
    const size_t total = (size_t)N * H * W;
    PROF_WORK(0, 5.0 * total);
    LAUNCH("hed", hed_nms_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, s, x, H, W, total, 127.0f, out);
    return 0;
}

int op_hed_blur_u8_bin(const unsigned char* src, int N, int H, int W, int out_channels, unsigned char* out, hipStream_t s) {
    CTRL_CHECK(src && out, "hed_blur_u8_bin: null pointer");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "hed_blur_u8_bin: out_channels must be 1 or 3");
    long tiles; int tx, ty;
    TRY(blur_dims("hed_blur_u8_bin", N, H, W, kTapsU8, &tiles, &tx, &ty));
    PROF_WORK(4.0 * kTapsU8 * N * H * W, (1.0 + out_channels) * N * H * W);
    LAUNCH("hed", (hed_blur_kernel<kTapsU8, true>), dim3((unsigned)tiles), dim3(NT), 0, s, src, H, W, tx, ty, gaussian_taps(kTapsU8), (float*)nullptr,
           out, out_channels);
    return 0;
}

int op_hed_scale_vec(float* v, int n, float scale, hipStream_t s) {
    CTRL_CHECK(v && n >= 1, "hed_scale_vec: bad arguments");
    LAUNCH("hed", hed_scale_vec_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, v, n, scale);
    return 0;
}
