// Lineart annotator (controlnet_aux LineartDetector over two Generator(3, 1, 3) nets: the reference's `lineart` condition,
// model/ctrl_helper.py:111-114, 190-191).  Activations fp16 NHWC, accumulation and statistics fp32.  The kernels around the implicit GEMMs:
//   stem        uint8 RGB frame -> / 255 -> reflect-3 gather -> 7x7 conv 3 -> 64 (K = 147) on the vector ALU in fp32 -> fp16 [N][H][W][64].
//               An 8 x 16 tile with its halo and the 147 x 64 weights sit in LDS; one thread owns four neighbouring pixels x eight channels
//   in_stats    InstanceNorm statistics: per (image, channel) sum and sum of squares of an fp16 map.  A workgroup reduces a fixed number of
//               rows (32768 / C) in a fixed order to one partial, in_stats_finish adds an image's partials in a fixed order: no atomics,
//               and a frame's sums do not depend on its batch
//   in_apply    y = (x - mean) * rstd [ReLU] [+ residual] -> fp16, plain or REFLECT-PADDED by 1 or 3: the producer writes the border
//               pixels, so the 3x3 convolutions behind a ReflectionPad2d(1) run as valid convolutions on the implicit GEMM unchanged
//   head        reflect-3 padded 64-channel map -> 7x7 conv to one channel + bias -> sigmoid -> 255 - uint8(min(255, 255 s)) in 1 or 3
//               channels (+ fp32 logits).  An 8 x 16 tile with its halo in LDS; the 3136-term dot product of a pixel is spread over the eight
//               lanes that hold its eight channel octets, each walking the 49 taps for four neighbouring pixels, and joined by three
//               xor-shuffles in a fixed order
//   pack_convT  ConvTranspose2d(3, stride 2, padding 1, output_padding 1) weights [Cin][Cout][3][3] -> the phase pack fp16 [4][Cout][4][Cin]
//               of the implicit GEMM's IG_CONV2D_PHASE form (zeros in the taps a phase does not use)
#include "ops.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int kTH = 8, kTW = 16;                 // output pixels of one workgroup of the stem and the head
constexpr int kSH = kTH + 6, kSW = kTW + 6;      // with the 7x7 halo
constexpr int kHeadPS = 72;                      // halves between pixels of the head's LDS tile: 144 B spreads the 16-byte chunks over the banks
typedef const h8* h8p;

__device__ __forceinline__ bool out_of_f16(float v) { return !(fabsf(v) <= 65504.0f); }
// index i of a map of n pixels under reflection (no edge repeat), for -n < i < 2n - 1; clamped so that a tile's overhang stays in bounds
__device__ __forceinline__ int reflect_clamped(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ---------------------------------------------------------------------------------------------------------------- stem
// w fp32 [49][3][64] (tap-major, the net's RGB order); grid: one workgroup per (frame, 8 x 16 tile)
__global__ __launch_bounds__(NT) void lineart_stem_kernel(const unsigned char* __restrict__ src, const float* __restrict__ w, int H, int W,
                                                          int tx, int ty, half_t* __restrict__ out, int32_t* nonfinite) {
    __shared__ __attribute__((aligned(16))) float sw[147 * 64];
    __shared__ float sx[kSH * kSW * 3];
    const int tile = blockIdx.x, n = tile / (tx * ty), tr = tile - n * tx * ty, y0 = (tr / tx) * kTH, x0 = (tr % tx) * kTW;
    for (int i = threadIdx.x; i < 147 * 64; i += NT) sw[i] = w[i];
    const unsigned char* img = src + (size_t)n * H * W * 3;
    for (int i = threadIdx.x; i < kSH * kSW * 3; i += NT) {
        const int c = i % 3, pix = i / 3, ly = pix / kSW, lx = pix - ly * kSW;
        const int gy = reflect_clamped(y0 + ly - 3, H), gx = reflect_clamped(x0 + lx - 3, W);
        sx[i] = (float)img[((size_t)gy * W + gx) * 3 + c] / 255.0f;
    }
    __syncthreads();
    const int cg = threadIdx.x & 7, q = threadIdx.x >> 3, qy = q >> 2, qx = (q & 3) * 4;
    float acc[4][8];
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[px][j] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
        float in[10][3];
        const float* row = sx + ((qy + ky) * kSW + qx) * 3;
#pragma unroll
        for (int i = 0; i < 30; ++i) in[i / 3][i % 3] = row[i];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* wk = sw + ((ky * 7 + kx) * 3 + c) * 64 + cg * 8;
                const f4 w0 = *(const f4*)wk, w1 = *(const f4*)(wk + 4);
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    const float v = in[px + kx][c];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[px][j] = fmaf(v, w0[j], acc[px][j]);
                        acc[px][4 + j] = fmaf(v, w1[j], acc[px][4 + j]);
                    }
                }
            }
    }
    const int y = y0 + qy;
    bool bad = false;
    if (y < H) {
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int x = x0 + qx + px;
            if (x >= W) continue;
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bad = bad || out_of_f16(acc[px][j]);
                o[j] = (half_t)acc[px][j];
            }
            *(h8*)(out + (((size_t)n * H + y) * W + x) * 64 + cg * 8) = o;
        }
    }
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;
}

// ---------------------------------------------------------------------------------------------------------------- InstanceNorm
// rows of one workgroup of the statistics pass: 64 KB of the map whatever its width
__host__ __device__ constexpr int in_rows_per_block(int C) { return 32768 / C; }

// grid (chunks, N).  A row's C / 8 octets lie on neighbouring lanes, 256 / (C / 8) rows are walked at once; the row slots are added through
// LDS in slot order.  partial [N][chunks][2][C]
__global__ __launch_bounds__(NT) void in_stats_kernel(const half_t* __restrict__ x, int HW, int C, float* __restrict__ partial) {
    __shared__ float red[2][NT * 8];
    const int L = C >> 3, R = NT / L, l = threadIdx.x % L, r = threadIdx.x / L;
    const int rpb = in_rows_per_block(C), row0 = blockIdx.x * rpb, row1 = min(row0 + rpb, HW);
    const half_t* img = x + (size_t)blockIdx.y * HW * C;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
    for (int row = row0 + r; row < row1; row += R) {
        const h8 v = *(h8p)(img + (size_t)row * C + l * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = (float)v[j];
            s[j] += f;
            q[j] = fmaf(f, f, q[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[0][r * C + l * 8 + j] = s[j];
        red[1][r * C + l * 8 + j] = q[j];
    }
    __syncthreads();
    float* dst = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += NT) {
        const int k = i / C, c = i - k * C;
        float a = 0.f;
        for (int rr = 0; rr < R; ++rr) a += red[k][rr * C + c];
        dst[i] = a;
    }
}

// grid (N): stats [N][C][2] = (sum, sum of squares); an image's partials in four interleaved chains, joined as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(NT) void in_stats_finish_kernel(const float* __restrict__ partial, int chunks, int C, float* __restrict__ stats) {
    const float* p = partial + (size_t)blockIdx.x * chunks * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += NT) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < chunks; ++k) a[k & 3] += p[(size_t)k * 2 * C + i];
        const int kk = i / C, c = i - kk * C;
        stats[((size_t)blockIdx.x * C + c) * 2 + kk] = (a[0] + a[1]) + (a[2] + a[3]);
    }
}

// one thread: eight channels of one OUTPUT pixel.  out [N][H + 2 pad][W + 2 pad][C]; res (optional) [N][H + 2 res_pad][W + 2 res_pad][C]
__global__ __launch_bounds__(NT) void in_apply_kernel(const half_t* __restrict__ x, const float* __restrict__ stats, const half_t* __restrict__ res,
                                                      int H, int W, int C8, int pad, int res_pad, int relu, float inv_count, float eps,
                                                      long total, half_t* __restrict__ out, int32_t* nonfinite) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int c8 = (int)(i % C8);
    long r = i / C8;
    const int ox = (int)(r % Wp); r /= Wp;
    const int oy = (int)(r % Hp);
    const long n = r / Hp;
    const int sy = reflect_clamped(oy - pad, H), sx = reflect_clamped(ox - pad, W);
    const h8 v = *(h8p)(x + (((size_t)n * H + sy) * W + sx) * (C8 * 8) + c8 * 8);
    const float* st = stats + ((size_t)n * C8 + c8) * 16;
    h8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (res) {
        const int Hr = H + 2 * res_pad, Wr = W + 2 * res_pad;
        rv = *(h8p)(res + (((size_t)n * Hr + sy + res_pad) * Wr + sx + res_pad) * (C8 * 8) + c8 * 8);
    }
    h8 o;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float mean = st[2 * j] * inv_count;
        const float var = fmaxf(fmaf(st[2 * j + 1], inv_count, -mean * mean), 0.f);
        float y = ((float)v[j] - mean) * rsqrtf(var + eps);
        if (relu) y = fmaxf(y, 0.f);
        y += (float)rv[j];
        bad = bad || out_of_f16(y);
        o[j] = (half_t)y;
    }
    *(h8*)(out + (size_t)i * 8) = o;
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;
}

// ---------------------------------------------------------------------------------------------------------------- head
// xp fp16 [N][H + 6][W + 6][64]; w fp32 [49][64]; grid: one workgroup per (frame, 8 x 16 tile)
template <int CH>
__global__ __launch_bounds__(NT) void lineart_head_kernel(const half_t* __restrict__ xp, const float* __restrict__ w, float bias, int H, int W,
                                                          int tx, int ty, unsigned char* __restrict__ out, float* __restrict__ logits) {
    __shared__ __attribute__((aligned(16))) half_t sx[kSH * kSW * kHeadPS];
    __shared__ __attribute__((aligned(16))) float sw[49 * 64];
    const int tile = blockIdx.x, n = tile / (tx * ty), tr = tile - n * tx * ty, y0 = (tr / tx) * kTH, x0 = (tr % tx) * kTW;
    const int Hp = H + 6, Wp = W + 6;
    for (int i = threadIdx.x; i < 49 * 64; i += NT) sw[i] = w[i];
    const half_t* img = xp + (size_t)n * Hp * Wp * 64;
    for (int i = threadIdx.x; i < kSH * kSW * 8; i += NT) {
        const int pix = i >> 3, c8 = i & 7, ly = pix / kSW, lx = pix - ly * kSW;
        const int gy = min(y0 + ly, Hp - 1), gx = min(x0 + lx, Wp - 1);      // (the clamp only serves a tile's overhang, which is not stored)
        *(h8*)(sx + pix * kHeadPS + c8 * 8) = *(h8p)(img + ((size_t)gy * Wp + gx) * 64 + c8 * 8);
    }
    __syncthreads();
    const int cg = threadIdx.x & 7, q = threadIdx.x >> 3, qy = q >> 2, qx = (q & 3) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
        h8 in[10];
        const half_t* row = sx + ((qy + ky) * kSW + qx) * kHeadPS + cg * 8;
#pragma unroll
        for (int i = 0; i < 10; ++i) in[i] = *(h8p)(row + i * kHeadPS);
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const float* wk = sw + (ky * 7 + kx) * 64 + cg * 8;
            const f4 w0 = *(const f4*)wk, w1 = *(const f4*)(wk + 4);
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const h8 v = in[px + kx];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[px] = fmaf((float)v[j], w0[j], acc[px]);
                    acc[px] = fmaf((float)v[4 + j], w1[j], acc[px]);
                }
            }
        }
    }
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        acc[px] += __shfl_xor(acc[px], 1, 64);
        acc[px] += __shfl_xor(acc[px], 2, 64);
        acc[px] += __shfl_xor(acc[px], 4, 64);
    }
    const int y = y0 + qy;
    if (cg != 0 || y >= H) return;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const int x = x0 + qx + px;
        if (x >= W) continue;
        const float z = acc[px] + bias;
        const float sg = 1.0f / (1.0f + expf(-z));
        const unsigned char b = (unsigned char)(255 - (int)fminf(255.0f, 255.0f * sg));      // truncation, then the inversion
        const size_t p = ((size_t)n * H + y) * W + x;
#pragma unroll
        for (int c = 0; c < CH; ++c) out[p * CH + c] = b;
        if (logits) logits[p] = z;
    }
}

// ---------------------------------------------------------------------------------------------------------------- transposed-conv pack
// out[ph = 2a + b][co][t = 2ty + tx][ci] = w[ci][co][ky][kx], (a, ty) -> ky: (0,0) none, (0,1) 1, (1,0) 2, (1,1) 0; the same for (b, tx) -> kx
__device__ __forceinline__ int convT_tap(int a, int t) { return a == 0 ? (t == 0 ? -1 : 1) : (t == 0 ? 2 : 0); }
__global__ void pack_convT_w_phase_kernel(const void* __restrict__ w, int dt, half_t* __restrict__ out, int Cin, int Cout, int* ovf) {
    const size_t per = (size_t)Cout * 4 * Cin, total = 4 * per;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        const size_t r = i / Cin;
        const int t = (int)(r & 3);
        const size_t co = (r >> 2) % Cout;
        const int ph = (int)(i / per);
        const int ky = convT_tap(ph >> 1, t >> 1), kx = convT_tap(ph & 1, t & 1);
        float v = 0.f;
        if (ky >= 0 && kx >= 0) v = load_as_f32(w, ((size_t)ci * Cout + co) * 9 + ky * 3 + kx, dt);
        if (ovf && !(fabsf(v) <= 65504.f)) *ovf = 1;
        out[i] = (half_t)v;
    }
}

int check_map(const char* what, int N, int H, int W, int per_pixel) {
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1, std::string(what) + ": N, H and W must be positive");
    CTRL_CHECK((double)N * H * W * per_pixel < 2147483648.0, std::string(what) + ": the batch must stay below 2^31 elements; split it");
    return 0;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// widths the InstanceNorm kernels take: whole octets per lane, a whole number of rows per 256 threads, a statistics tile that fits LDS
bool in_width_ok(int C) { return C >= 8 && C <= 256 && C % 8 == 0 && NT % (C / 8) == 0; }

}  // namespace

void lineart_launch_shape(int kernel, int C, int* a, int* b) {
    if (kernel == 2) { *a = in_rows_per_block(C); *b = 1; }
    else { *a = kTH; *b = kTW; }
}

int op_lineart_stem(const unsigned char* src, int N, int H, int W, const float* w, half_t* out, int32_t* nonfinite, hipStream_t s) {
    CTRL_CHECK(src && w && out, "lineart_stem: null pointer");
    TRY(check_map("lineart_stem", N, H, W, 64));
    CTRL_CHECK(H >= 4 && W >= 4, "lineart_stem: reflection padding by 3 needs H and W of at least 4");
    CTRL_CHECK(aligned16(out), "lineart_stem: out must be 16-byte aligned");
    const int tx = (W + kTW - 1) / kTW, ty = (H + kTH - 1) / kTH;
    PROF_WORK(2.0 * 147 * 64 * N * H * W, (double)N * H * W * (3 + 128));
    prof_detail("N%d %dx%d", N, H, W);
    LAUNCH("lineart_stem", lineart_stem_kernel, dim3((unsigned)((long)N * tx * ty)), dim3(NT), 0, s, src, w, H, W, tx, ty, out, nonfinite);
    return 0;
}

size_t op_in_stats_ws_floats(int N, int HW, int C) {
    if (N < 1 || HW < 1 || !in_width_ok(C)) return 0;
    const int rpb = in_rows_per_block(C);
    return (size_t)N * ((HW + rpb - 1) / rpb) * 2 * C;
}

int op_in_stats(const half_t* x, int N, int HW, int C, float* stats, float* ws, hipStream_t s) {
    CTRL_CHECK(x && stats && ws, "in_stats: null pointer");
    CTRL_CHECK(in_width_ok(C), "in_stats: C must be 8, 16, 32, 64, 128 or 256");
    CTRL_CHECK(N >= 1 && N <= 65535 && HW >= 1 && (double)N * HW * C < 2147483648.0, "in_stats: 1..65535 images, below 2^31 elements");
    CTRL_CHECK(aligned16(x), "in_stats: x must be 16-byte aligned");
    const int rpb = in_rows_per_block(C), chunks = (HW + rpb - 1) / rpb;
    PROF_WORK(3.0 * N * HW * C, 2.0 * N * HW * C);
    prof_detail("N%d HW%d C%d", N, HW, C);
    LAUNCH("in_stats", in_stats_kernel, dim3(chunks, N), dim3(NT), 0, s, x, HW, C, ws);
    LAUNCH("in_stats", in_stats_finish_kernel, dim3(N), dim3(NT), 0, s, (const float*)ws, chunks, C, stats);
    return 0;
}

int op_in_apply(const half_t* x, const float* stats, int N, int H, int W, int C, float eps, int relu, const half_t* res, int res_pad, int pad,
                half_t* out, int32_t* nonfinite, hipStream_t s) {
    CTRL_CHECK(x && stats && out, "in_apply: null pointer");
    CTRL_CHECK(in_width_ok(C), "in_apply: C must be 8, 16, 32, 64, 128 or 256");
    CTRL_CHECK(pad == 0 || pad == 1 || pad == 3, "in_apply: the output is plain (0) or reflect-padded by 1 or 3");
    CTRL_CHECK(!res || res_pad == 0 || res_pad == 1 || res_pad == 3, "in_apply: the residual is plain (0) or reflect-padded by 1 or 3");
    CTRL_CHECK(N >= 1 && H > pad && W > pad, "in_apply: reflection padding by p needs H and W above p");
    CTRL_CHECK((double)N * (H + 6) * (W + 6) * C < 2147483648.0, "in_apply: the batch must stay below 2^31 elements; split it");
    CTRL_CHECK(aligned16(x) && aligned16(out) && aligned16(res) && aligned16(stats), "in_apply: pointers must be 16-byte aligned");
    const long total = (long)N * (H + 2 * pad) * (W + 2 * pad) * (C / 8);
    PROF_WORK(4.0 * total * 8, 2.0 * 8 * total * (res ? 3 : 2));
    prof_detail("N%d %dx%d C%d pad%d%s%s", N, H, W, C, pad, relu ? " relu" : "", res ? " res" : "");
    LAUNCH("in_apply", in_apply_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, s, x, stats, res, H, W, C / 8, pad, res ? res_pad : 0,
           relu ? 1 : 0, 1.0f / ((float)H * (float)W), eps, total, out, nonfinite);
    return 0;
}

int op_lineart_head(const half_t* xp, int N, int H, int W, const float* w, float bias, int out_channels, unsigned char* out, float* logits,
                    hipStream_t s) {
    CTRL_CHECK(xp && w && out, "lineart_head: null pointer");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "lineart_head: out_channels must be 1 or 3");
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1 && (double)N * (H + 6) * (W + 6) * 64 < 2147483648.0, "lineart_head: the batch must stay below 2^31 elements; split it");
    CTRL_CHECK(aligned16(xp), "lineart_head: the operand must be 16-byte aligned");
    const int tx = (W + kTW - 1) / kTW, ty = (H + kTH - 1) / kTH;
    const dim3 grid((unsigned)((long)N * tx * ty));
    PROF_WORK(2.0 * 3136 * N * H * W, (double)N * (H + 6) * (W + 6) * 128 + (double)N * H * W * (out_channels + (logits ? 4 : 0)));
    prof_detail("N%d %dx%d ch%d", N, H, W, out_channels);
    if (out_channels == 3) LAUNCH("lineart_head", lineart_head_kernel<3>, grid, dim3(NT), 0, s, xp, w, bias, H, W, tx, ty, out, logits);
    else LAUNCH("lineart_head", lineart_head_kernel<1>, grid, dim3(NT), 0, s, xp, w, bias, H, W, tx, ty, out, logits);
    return 0;
}

int op_pack_convT_w_phase(const void* w, int dtype, half_t* out, int Cin, int Cout, hipStream_t s, int* ovf) {
    CTRL_CHECK(w && out, "pack_convT_w_phase: null pointer");
    CTRL_CHECK(dtype >= DT_F32 && dtype <= DT_BF16, "pack_convT_w_phase: the source must be fp32, fp16 or bf16");
    CTRL_CHECK(Cin >= 1 && Cout >= 1 && 16.0 * Cin * Cout < 2147483648.0, "pack_convT_w_phase: every extent must be at least 1, below 2^31 elements");
    const size_t total = (size_t)16 * Cin * Cout;
    LAUNCH("pack", pack_convT_w_phase_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, w, dtype, out, Cin, Cout,
           ovf);
    return 0;
}
