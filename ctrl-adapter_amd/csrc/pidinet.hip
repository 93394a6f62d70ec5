// PiDiNet annotator (controlnet_aux PidiNetDetector, pidinet() = PiDiNet(60, 'carv4', dil 24, sa): the reference's `softedge` condition,
// model/ctrl_helper.py:103-107, 184-185).  Activations fp16 NHWC, channels padded 60 -> 64, 120 -> 128, 240 -> 256 (pad channels hold
// exact zeros: every weight is zero-padded, and a kernel that reads channels as values zeroes the pad while it stages), accumulation fp32.
//   stem          uint8 RGB frame -> BGR / 255 -> the converted `cd` 3x3 (3 -> 60, K = 27) on the vector ALU -> fp16
//   block         ONE launch per PDC block: a tile of x with its halo in LDS (max-pooled while loading in the stride-2 form), the converted
//                 depthwise kernel + ReLU on the vector ALU, its fp16 result through LDS as the MFMA operand of the 1x1 against the
//                 [cout][cin] weights, the skip (identity from the staged tile, or the shortcut's 1x1 as further k-steps of the same
//                 accumulators, plus its bias), fp16 store.  64 input channels at a time: the depthwise result never reaches HBM.
//   head_reduce   relu -> 1x1 C -> 24 (+ bias) on MFMA -> t fp16, 32 channels per pixel
//   head_context  a 16 x 16 tile of t with its 11-pixel halo in LDS, the four dilated 3x3 convolutions (36 taps x 32-deep k-steps) summed
//                 in one set of fp32 accumulators; the epilogue keeps the sums in registers and writes five fp32 per pixel:
//                 a4 = W_att1 . relu(s) + b_att1 and d = w_red . s   (MapReduce(CSAM(s)) = sigmoid(conv3x3(a4)) * d + b_red)
//   side          3x3 over a4 (zero padding), sigmoid, * d + b -> e fp32 at the stage's resolution
//   fuse          e1..e4 -> torch's bilinear (half-pixel centres, negative source coordinates clamped to 0) -> classifier -> sigmoid ->
//                 optional > 0.5 -> * 255, clip, truncate -> uint8 in 1 or 3 channels (+ fp32 logits)
// MFMA operand order as in smallconv.hip: D = W . X^T, so a lane ends with four consecutive output channels of one pixel.
#include "ops.h"
#include <cmath>
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int kBlockTH = 8, kBlockTW = 16;       // output pixels of one workgroup of the block kernel
constexpr int kHeadTS = 16, kHeadHalo = 11;      // the context head's tile and halo (the largest dilation)
typedef const h8* h8p;

__device__ __forceinline__ bool out_of_f16(float v) { return !(fabsf(v) <= 65504.0f); }

// ---------------------------------------------------------------------------------------------------------------- stem
// one thread: four neighbouring pixels of a row x eight output channels; the 27 x 64 weights sit in LDS (hed_stem_kernel's shape)
__global__ __launch_bounds__(NT) void pidi_stem_kernel(const unsigned char* __restrict__ src, const float* __restrict__ w, int H, int W,
                                                       long quads, half_t* __restrict__ out, int32_t* nonfinite) {
    __shared__ __attribute__((aligned(16))) float sw[27 * 64];
    for (int i = threadIdx.x; i < 27 * 64; i += NT) sw[i] = w[i];
    __syncthreads();
    const int cg = threadIdx.x & 7;
    const long q = (long)blockIdx.x * (NT / 8) + (threadIdx.x >> 3);
    if (q >= quads) return;
    const int wq = W >> 2;
    const long row = q / wq;                       // n * H + y
    const int x0 = (int)(q - row * wq) * 4, y = (int)(row % H);
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
            for (int c = 0; c < 3; ++c) in[dy][dx][c] = inb ? (float)p[2 - c] / 255.0f : 0.f;      // the net sees BGR
        }
    }
    float acc[4][8];
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[px][j] = 0.f;
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
            bad = bad || out_of_f16(acc[px][j]);
            o[j] = (half_t)acc[px][j];
        }
        *(h8*)(out + ((size_t)row * W + x0 + px) * 64 + cg * 8) = o;
    }
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;
}

// ---------------------------------------------------------------------------------------------------------------- PDC block
// which of the KS x KS positions the converted kernel can hold a weight at: all nine of a 3 x 3; of rd's 5 x 5 the inner ring and the
// eight compass points of the outer one
__host__ __device__ constexpr bool pidi_tap_used(int KS, int t) {
    if (KS == 3) return true;
    const int y = t / 5, x = t % 5;
    const int ay = y < 2 ? 2 - y : y - 2, ax = x < 2 ? 2 - x : x - 2;
    const int m = ay > ax ? ay : ax;
    return m == 1 || (m == 2 && ay != 1 && ax != 1);
}

// grid: one workgroup per (frame, 8 x 16 output tile).  Per 64 input channels: stage -> depthwise + ReLU -> fp16 tile in LDS -> two
// 32-deep k-steps of v_mfma_f32_16x16x32_f16.  Wave w owns the output channels [w * COUTP / 4, (w + 1) * COUTP / 4) of all eight pixel rows:
// a weight fragment is fetched once per workgroup and feeds eight MFMAs.
template <int CINP, int COUTP, int R, bool POOL>
__global__ __launch_bounds__(NT) void pidi_block_kernel(const half_t* __restrict__ x, const float* __restrict__ dw, const half_t* __restrict__ w2,
                                                        const half_t* __restrict__ wsc, const float* __restrict__ bsc, int C, int Hs, int Ws,
                                                        int H, int W, int tx, int ty, half_t* __restrict__ out, int32_t* nonfinite) {
    constexpr int TH = kBlockTH, TW = kBlockTW, KS = 2 * R + 1, SH = TH + 2 * R, SW = TW + 2 * R;
    constexpr int PS = 72;                          // halves between pixels in LDS: 144 B, so sixteen pixels' 16-byte chunks spread over the banks
    constexpr int NCH = CINP / 64, NF = COUTP / 64;
    __shared__ __attribute__((aligned(16))) half_t sx[SH * SW * PS];
    __shared__ __attribute__((aligned(16))) half_t sa[TH * TW * PS];
    __shared__ __attribute__((aligned(16))) float sdw[KS * KS * 64];
    const int tile = blockIdx.x, n = tile / (tx * ty), tr = tile - n * tx * ty, y0 = (tr / tx) * TH, x0 = (tr % tx) * TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, q = lane >> 4;
    const half_t* xin = x + (size_t)n * Hs * Ws * CINP;
    const h8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    f4 acc[TH][NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const f4 b = POOL ? *(const f4*)(bsc + (wave * NF + j) * 16 + q * 4) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < TH; ++m) acc[m][j] = b;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c) __syncthreads();                     // the previous chunk's MFMAs have read sx and sa
        for (int i = threadIdx.x; i < SH * SW * 8; i += NT) {
            const int pix = i >> 3, cg = i & 7, ly = pix / SW, lx = pix - ly * SW, gy = y0 + ly - R, gx = x0 + lx - R;
            h8 v = hz;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int ch0 = c * 64 + cg * 8;
                if (POOL) {
                    const half_t* b = xin + ((size_t)(2 * gy) * Ws + 2 * gx) * CINP + ch0;
                    const h8 v0 = *(h8p)b, v1 = *(h8p)(b + CINP), v2 = *(h8p)(b + (size_t)Ws * CINP), v3 = *(h8p)(b + (size_t)Ws * CINP + CINP);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const half_t a = v0[j] > v1[j] ? v0[j] : v1[j], e = v2[j] > v3[j] ? v2[j] : v3[j];
                        v[j] = a > e ? a : e;
                    }
                } else {
                    v = *(h8p)(xin + ((size_t)gy * Ws + gx) * CINP + ch0);
                }
                const int left = C - ch0;           // what the input's pad channels hold is not a value
                if (left < 8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = j < left ? v[j] : (half_t)0;
                }
            }
            *(h8*)(sx + pix * PS + cg * 8) = v;
        }
        for (int i = threadIdx.x; i < KS * KS * 64; i += NT) sdw[i] = dw[(size_t)(i >> 6) * CINP + c * 64 + (i & 63)];
        __syncthreads();
        {   // depthwise + ReLU: a thread takes eight channels of the pixels pg, pg + 32, pg + 64, pg + 96 of the tile
            const int cg = threadIdx.x & 7, pg = threadIdx.x >> 3;
            float a[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) a[k][j] = 0.f;
#pragma unroll
            for (int t = 0; t < KS * KS; ++t) {
                if (!pidi_tap_used(KS, t)) continue;
                const int ky = t / KS, kx = t % KS;
                const f4 w0 = *(const f4*)(sdw + t * 64 + cg * 8), w1 = *(const f4*)(sdw + t * 64 + cg * 8 + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pix = pg + 32 * k, py = pix >> 4, px = pix & 15;
                    const h8 v = *(h8p)(sx + ((py + ky) * SW + px + kx) * PS + cg * 8);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a[k][j] = fmaf((float)v[j], w0[j], a[k][j]);
                        a[k][4 + j] = fmaf((float)v[4 + j], w1[j], a[k][4 + j]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                h8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (half_t)(a[k][j] > 0.f ? a[k][j] : 0.f);
                *(h8*)(sa + (pg + 32 * k) * PS + cg * 8) = o;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k0 = c * 64 + ks * 32 + q * 8;
            h8 wf[NF], ws[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                wf[j] = *(h8p)(w2 + (size_t)((wave * NF + j) * 16 + p) * CINP + k0);
                if (POOL) ws[j] = *(h8p)(wsc + (size_t)((wave * NF + j) * 16 + p) * CINP + k0);
            }
#pragma unroll
            for (int m = 0; m < TH; ++m) {
                const h8 b = *(h8p)(sa + (m * TW + p) * PS + ks * 32 + q * 8);
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], b, acc[m][j], 0, 0, 0);
                if (POOL) {
                    const h8 bx = *(h8p)(sx + ((m + R) * SW + p + R) * PS + ks * 32 + q * 8);
#pragma unroll
                    for (int j = 0; j < NF; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[j], bx, acc[m][j], 0, 0, 0);
                }
            }
        }
        if (!POOL && c == (wave * NF) / 4) {        // the identity skip of this wave's output channels, from the staged tile (wave-uniform)
#pragma unroll
            for (int m = 0; m < TH; ++m)
#pragma unroll
                for (int j = 0; j < NF; ++j) {
                    const h4 v = *(const h4*)(sx + ((m + R) * SW + p + R) * PS + ((wave * NF + j) & 3) * 16 + q * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[m][j][i] += (float)v[i];
                }
        }
    }
    bool bad = false;
    const int gx = x0 + p;
#pragma unroll
    for (int m = 0; m < TH; ++m) {
        const int gy = y0 + m;
        if (gy < H && gx < W) {
            half_t* op = out + (((size_t)n * H + gy) * W + gx) * COUTP + q * 4;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const f4 v = acc[m][j];
                bad = bad || out_of_f16(v[0]) || out_of_f16(v[1]) || out_of_f16(v[2]) || out_of_f16(v[3]);
                const h4 o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                *(h4*)(op + (wave * NF + j) * 16) = o;
            }
        }
    }
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;
}

// ---------------------------------------------------------------------------------------------------------------- context head
// t = W1 . relu(x) + b1: a wave takes sixteen pixels, a lane fetches its 16-byte chunk of one pixel straight from global memory
template <int CP>
__global__ __launch_bounds__(NT) void pidi_head_reduce_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w1,
                                                              const float* __restrict__ b1, int C, long npix, half_t* __restrict__ t,
                                                              int32_t* nonfinite) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, q = lane >> 4;
    const long frag = (long)blockIdx.x * 4 + wave;
    if (frag * 16 >= npix) return;                  // (a whole wave leaves)
    const long pix = frag * 16 + p;
    const bool ok = pix < npix;
    const h8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    f4 acc[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[f] = *(const f4*)(b1 + f * 16 + q * 4);
#pragma unroll
    for (int ks = 0; ks < CP / 32; ++ks) {
        const int k0 = ks * 32 + q * 8;
        h8 b = ok ? *(h8p)(x + (size_t)pix * CP + k0) : hz;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (b[j] > (half_t)0 && k0 + j < C) ? b[j] : (half_t)0;
#pragma unroll
        for (int f = 0; f < 2; ++f)
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(h8p)(w1 + (size_t)(f * 16 + p) * CP + k0), b, acc[f], 0, 0, 0);
    }
    bool bad = false;
    if (ok) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const f4 v = acc[f];
            bad = bad || out_of_f16(v[0]) || out_of_f16(v[1]) || out_of_f16(v[2]) || out_of_f16(v[3]);
            const h4 o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *(h4*)(t + (size_t)pix * kPidiHeadCP + f * 16 + q * 4) = o;
        }
    }
    if (nonfinite && bad) *(volatile int32_t*)nonfinite = 1;
}

struct HeadPar { float v[124]; };                   // att [4][24] | att_b [4] | red [24]

// grid: one workgroup per (frame, 16 x 16 tile); dynamic LDS: the tile of t with its halo, 38 x 38 pixels x 80 B.  Wave w owns the tile's
// rows 4 w .. 4 w + 3 (one 16-pixel fragment each) x both 16-channel fragments of the 24 (+ 8 zero) outputs.
__global__ __launch_bounds__(NT) void pidi_head_context_kernel(const half_t* __restrict__ t, const half_t* __restrict__ wd, HeadPar par, int H,
                                                               int W, int tx, int ty, float* __restrict__ a4, float* __restrict__ d) {
    constexpr int TS = kHeadTS, HL = kHeadHalo, SW = TS + 2 * HL, PS = 40, CPH = kPidiHeadCP;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    half_t* st = (half_t*)smem_raw;
    __shared__ float spar[124];
    const int tile = blockIdx.x, n = tile / (tx * ty), tr = tile - n * tx * ty, y0 = (tr / tx) * TS, x0 = (tr % tx) * TS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, q = lane >> 4;
    const half_t* tin = t + (size_t)n * H * W * CPH;
    const h8 hz = {0, 0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 124; ++i) spar[i] = par.v[i];
    }
    for (int i = threadIdx.x; i < SW * SW * 4; i += NT) {
        const int pix = i >> 2, cg = i & 3, ly = pix / SW, lx = pix - ly * SW, gy = y0 + ly - HL, gx = x0 + lx - HL;
        const bool inb = gy >= 0 && gy < H && gx >= 0 && gx < W;
        *(h8*)(st + pix * PS + cg * 8) = inb ? *(h8p)(tin + ((size_t)gy * W + gx) * CPH + cg * 8) : hz;
    }
    __syncthreads();
    f4 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[r][f] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int di = 0; di < 4; ++di) {
        const int dil = 5 + 2 * di;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int oy = (k / 3 - 1) * dil, ox = (k % 3 - 1) * dil, tap = di * 9 + k;
            const h8 w0 = *(h8p)(wd + ((size_t)tap * CPH + p) * CPH + q * 8), w1 = *(h8p)(wd + ((size_t)tap * CPH + 16 + p) * CPH + q * 8);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const h8 b = *(h8p)(st + ((wave * 4 + r + HL + oy) * SW + p + HL + ox) * PS + q * 8);
                acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, b, acc[r][0], 0, 0, 0);
                acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, b, acc[r][1], 0, 0, 0);
            }
        }
    }
    // a lane holds s of the channels f * 16 + q * 4 + i of pixel (4 wave + r, p): partial dot products, summed over the four q lanes
    const int gx = x0 + p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float pa[4] = {0.f, 0.f, 0.f, 0.f}, pd = 0.f;
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = f * 16 + q * 4 + i;
                if (c < kPidiHeadC) {
                    const float s = acc[r][f][i], rs = s > 0.f ? s : 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) pa[k] = fmaf(spar[k * 24 + c], rs, pa[k]);
                    pd = fmaf(spar[100 + c], s, pd);
                }
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pa[k] += __shfl_xor(pa[k], 16, 64);
            pa[k] += __shfl_xor(pa[k], 32, 64);
        }
        pd += __shfl_xor(pd, 16, 64);
        pd += __shfl_xor(pd, 32, 64);
        const int gy = y0 + wave * 4 + r;
        if (q == 0 && gy < H && gx < W) {
            const size_t o = ((size_t)n * H + gy) * W + gx;
            *(f4*)(a4 + o * 4) = f4{pa[0] + spar[96], pa[1] + spar[97], pa[2] + spar[98], pa[3] + spar[99]};
            d[o] = pd;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- side map
struct SidePar { float w[36]; float b; };           // w [ky][kx][4]

__global__ __launch_bounds__(NT) void pidi_side_kernel(const float* __restrict__ a4, const float* __restrict__ d, SidePar par, int H, int W,
                                                       size_t total, float* __restrict__ e) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int px = (int)(i % W), py = (int)((i / W) % H);
    const float* img = a4 + (i - (size_t)py * W - px) * 4;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = py + ky - 1, xx = px + kx - 1;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const f4 v = *(const f4*)(img + ((size_t)yy * W + xx) * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fmaf(par.w[(ky * 3 + kx) * 4 + c], v[c], acc);
            }
        }
    e[i] = fmaf(1.0f / (1.0f + expf(-acc)), d[i], par.b);
}

// ---------------------------------------------------------------------------------------------------------------- fuse
struct FusePar { const float* p[4]; float w[4]; float b; };

// torch's upsample_bilinear2d, align_corners = False: src = (dst + 0.5) * scale - 0.5, negative values clamped to 0, i1 = i0 + 1 inside
__device__ __forceinline__ void torch_coord(int dst, float sc, int n, int* i0, int* i1, float* l1) {
    float src = ((float)dst + 0.5f) * sc - 0.5f;
    src = src < 0.f ? 0.f : src;
    int a = (int)src;
    a = a < n - 1 ? a : n - 1;
    *i0 = a; *i1 = a < n - 1 ? a + 1 : a; *l1 = src - (float)a;
}

template <int CH>
__global__ __launch_bounds__(NT) void pidi_fuse_kernel(FusePar m, int H, int W, long quads, int filter, unsigned char* __restrict__ out,
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
        float lg = fmaf(m.w[0], m.p[0][(size_t)row * W + x], m.b);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const int hk = H >> k, wk = W >> k;
            const float sc = 1.0f / (float)(1 << k);
            int xa, xb, ya, yb;
            float fx, fy;
            torch_coord(x, sc, wk, &xa, &xb, &fx);
            torch_coord(y, sc, hk, &ya, &yb, &fy);
            const float* P = m.p[k] + (size_t)n * hk * wk;
            const float r0 = (1.f - fx) * P[ya * wk + xa] + fx * P[ya * wk + xb];
            const float r1 = (1.f - fx) * P[yb * wk + xa] + fx * P[yb * wk + xb];
            lg = fmaf(m.w[k], (1.f - fy) * r0 + fy * r1, lg);
        }
        if (logit) logit[(size_t)row * W + x] = lg;
        float u = 1.0f / (1.0f + expf(-lg));
        if (filter) u = u > 0.5f ? 1.f : 0.f;
        u *= 255.0f;
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

int check_map(const char* what, int N, int H, int W, int per_pixel) {
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1, std::string(what) + ": N, H and W must be positive");
    CTRL_CHECK((double)N * H * W * per_pixel < 2147483648.0, std::string(what) + ": the batch must stay below 2^31 elements; split it");
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int CINP, int COUTP>
int launch_block(const half_t* x, int N, int H, int W, int Cin, int taps, const float* dw, const half_t* w2, const half_t* wsc, const float* bsc,
                 int pool, half_t* out, int32_t* flag, hipStream_t s) {
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    const int tx = (Wo + kBlockTW - 1) / kBlockTW, ty = (Ho + kBlockTH - 1) / kBlockTH;
    const dim3 grid((unsigned)((long)N * tx * ty));
    PROF_WORK(2.0 * N * Ho * Wo * CINP * (taps + (pool ? 2.0 : 1.0) * COUTP), 2.0 * ((double)N * H * W * CINP + (double)N * Ho * Wo * COUTP));
    prof_detail("N%d %d->%d %dx%d taps%d%s", N, CINP, COUTP, H, W, taps, pool ? " pool" : "");
#define PIDI_BLOCK(RR, PP) LAUNCH("pidi_block", (pidi_block_kernel<CINP, COUTP, RR, PP>), grid, dim3(NT), 0, s, x, dw, w2, wsc, bsc, Cin, H, W, \
                                  Ho, Wo, tx, ty, out, flag)
    if (taps == 9 && !pool) PIDI_BLOCK(1, false);
    else if (taps == 9) PIDI_BLOCK(1, true);
    else if (!pool) PIDI_BLOCK(2, false);
    else PIDI_BLOCK(2, true);
#undef PIDI_BLOCK
    return 0;
}

}  // namespace

void pidi_launch_shape(int kernel, int* tile_h, int* tile_w) {
    *tile_h = kernel == 0 ? kBlockTH : kHeadTS;
    *tile_w = kernel == 0 ? kBlockTW : kHeadTS;
}

// host: the vanilla kernel of a pixel-difference convolution (PiDiNet's ops.py createConvFunc), per [Co][Ci] plane of nine weights
int pidi_convert_pdc(int kind, const float* w, int Co, int Ci, float* out) {
    CTRL_CHECK(w && out && Co >= 1 && Ci >= 1, "pidi_convert_pdc: bad arguments");
    CTRL_CHECK(kind >= 0 && kind <= 3, "pidi_convert_pdc: kind must be 0 (cv), 1 (cd), 2 (ad) or 3 (rd)");
    static const int ad_from[9] = {3, 0, 1, 6, 4, 2, 7, 8, 5};
    static const int rd_pos[8] = {0, 2, 4, 10, 14, 20, 22, 24}, rd_neg[8] = {6, 7, 8, 11, 13, 16, 17, 18};
    for (long pl = 0; pl < (long)Co * Ci; ++pl) {
        const float* f = w + pl * 9;
        if (kind == 3) {
            float* b = out + pl * 25;
            for (int i = 0; i < 25; ++i) b[i] = 0.f;
            for (int i = 0; i < 8; ++i) {
                b[rd_pos[i]] = f[i + 1];
                b[rd_neg[i]] = (float)(-(double)f[i + 1]);
            }
            continue;
        }
        float* o = out + pl * 9;
        double sum = 0.0;
        for (int i = 0; i < 9; ++i) sum += (double)f[i];
        for (int i = 0; i < 9; ++i) {
            double v = (double)f[i];
            if (kind == 1 && i == 4) v -= sum;
            if (kind == 2) v -= (double)f[ad_from[i]];
            o[i] = (float)v;
        }
    }
    return 0;
}

int op_pidi_stem(const unsigned char* src, int N, int H, int W, const float* w, half_t* out, int32_t* nonfinite, hipStream_t s) {
    CTRL_CHECK(src && w && out, "pidi_stem: null pointer");
    TRY(check_map("pidi_stem", N, H, W, 64));
    CTRL_CHECK(W % 4 == 0, "pidi_stem: W must be a multiple of 4");
    CTRL_CHECK(aligned16(out) && aligned16(w), "pidi_stem: w and out must be 16-byte aligned");
    const long quads = (long)N * H * W / 4;
    PROF_WORK(2.0 * 27 * 64 * N * H * W, (double)N * H * W * (3 + 128));
    prof_detail("N%d %dx%d", N, H, W);
    LAUNCH("pidi", pidi_stem_kernel, dim3((unsigned)((quads + NT / 8 - 1) / (NT / 8))), dim3(NT), 0, s, src, w, H, W, quads, out, nonfinite);
    return 0;
}

int op_pidi_block(const half_t* x, int N, int H, int W, int Cin, int Cout, int taps, const float* dw, const half_t* w2, const half_t* wsc,
                  const float* bsc, int pool, half_t* out, int32_t* nonfinite, hipStream_t s) {
    CTRL_CHECK(x && dw && w2 && out, "pidi_block: null pointer");
    CTRL_CHECK(taps == 9 || taps == 25, "pidi_block: taps must be 9 or 25");
    CTRL_CHECK(Cin >= 1 && Cout >= 1 && Cin <= 256 && Cout <= 256 && Cin % 4 == 0 && Cout % 4 == 0, "pidi_block: Cin and Cout must be multiples of 4, at most 256");
    const int cip = pidi_cp(Cin), cop = pidi_cp(Cout);
    TRY(check_map("pidi_block", N, H, W, cip > cop ? cip : cop));
    CTRL_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), "pidi_block: the pooled form needs even H and W");
    CTRL_CHECK((wsc != nullptr) == (pool != 0) && (wsc == nullptr) == (bsc == nullptr),
               "pidi_block: the shortcut (wsc and bsc) goes with pool = 1, the identity skip with pool = 0");
    CTRL_CHECK(pool || Cin == Cout, "pidi_block: the identity skip needs Cin == Cout");
    CTRL_CHECK(aligned16(x) && aligned16(out) && aligned16(w2) && aligned16(dw) && aligned16(wsc) && aligned16(bsc),
               "pidi_block: pointers must be 16-byte aligned");
#define PIDI_W(CI, CO) if (cip == CI && cop == CO) return launch_block<CI, CO>(x, N, H, W, Cin, taps, dw, w2, wsc, bsc, pool, out, nonfinite, s)
    PIDI_W(64, 64);
    PIDI_W(128, 128);
    PIDI_W(256, 256);
    PIDI_W(64, 128);
    PIDI_W(128, 256);
#undef PIDI_W
    CTRL_FAIL("pidi_block: unsupported widths " + std::to_string(Cin) + " -> " + std::to_string(Cout) +
              " (padded 64 -> 64 | 128, 128 -> 128 | 256, 256 -> 256)");
}

int op_pidi_head_reduce(const half_t* x, int N, int H, int W, int C, const half_t* w1, const float* b1, half_t* t, int32_t* nonfinite,
                        hipStream_t s) {
    CTRL_CHECK(x && w1 && b1 && t, "pidi_head_reduce: null pointer");
    CTRL_CHECK(C >= 1 && C <= 256, "pidi_head_reduce: C must be at most 256");
    const int cp = pidi_cp(C);
    TRY(check_map("pidi_head_reduce", N, H, W, cp));
    CTRL_CHECK(aligned16(x) && aligned16(w1) && aligned16(b1) && aligned16(t), "pidi_head_reduce: pointers must be 16-byte aligned");
    const long npix = (long)N * H * W;
    const dim3 grid((unsigned)((npix + 63) / 64));
    PROF_WORK(2.0 * npix * cp * kPidiHeadCP, (double)npix * 2.0 * (cp + kPidiHeadCP));
    prof_detail("N%d C%d %dx%d", N, cp, H, W);
    if (cp == 64) LAUNCH("pidi_head", pidi_head_reduce_kernel<64>, grid, dim3(NT), 0, s, x, w1, b1, C, npix, t, nonfinite);
    else if (cp == 128) LAUNCH("pidi_head", pidi_head_reduce_kernel<128>, grid, dim3(NT), 0, s, x, w1, b1, C, npix, t, nonfinite);
    else LAUNCH("pidi_head", pidi_head_reduce_kernel<256>, grid, dim3(NT), 0, s, x, w1, b1, C, npix, t, nonfinite);
    return 0;
}

int op_pidi_head_context(const half_t* t, int N, int H, int W, const half_t* wd, const float* par124, float* a4, float* d, hipStream_t s) {
    CTRL_CHECK(t && wd && par124 && a4 && d, "pidi_head_context: null pointer");
    TRY(check_map("pidi_head_context", N, H, W, kPidiHeadCP));
    CTRL_CHECK(aligned16(t) && aligned16(wd) && aligned16(a4), "pidi_head_context: pointers must be 16-byte aligned");
    constexpr int SW = kHeadTS + 2 * kHeadHalo;
    constexpr size_t smem = (size_t)SW * SW * 40 * sizeof(half_t);
    static bool attr_set[kMaxDevices] = {};
    const int dev = cur_device();
    if (!attr_set[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void*)pidi_head_context_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        attr_set[dev] = true;
    }
    HeadPar par;
    for (int i = 0; i < 124; ++i) par.v[i] = par124[i];
    const int tx = (W + kHeadTS - 1) / kHeadTS, ty = (H + kHeadTS - 1) / kHeadTS;
    PROF_WORK(2.0 * N * H * W * kPidiHeadTaps * kPidiHeadCP * kPidiHeadCP, (double)N * H * W * (2.0 * kPidiHeadCP + 20.0));
    prof_detail("N%d %dx%d", N, H, W);
    LAUNCH("pidi_head", pidi_head_context_kernel, dim3((unsigned)((long)N * tx * ty)), dim3(NT), smem, s, t, wd, par, H, W, tx, ty, a4, d);
    return 0;
}

int op_pidi_side(const float* a4, const float* d, int N, int H, int W, const float* par37, float* e, hipStream_t s) {
    CTRL_CHECK(a4 && d && par37 && e, "pidi_side: null pointer");
    TRY(check_map("pidi_side", N, H, W, 4));
    CTRL_CHECK(aligned16(a4), "pidi_side: a4 must be 16-byte aligned");
    SidePar par;
    for (int i = 0; i < 36; ++i) par.w[i] = par37[i];
    par.b = par37[36];
    const size_t total = (size_t)N * H * W;
    PROF_WORK(2.0 * 36 * total, 24.0 * total);
    prof_detail("N%d %dx%d", N, H, W);
    LAUNCH("pidi", pidi_side_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, s, a4, d, par, H, W, total, e);
    return 0;
}

int op_pidi_fuse(const float* const* maps4, int N, int H, int W, const float* par5, int apply_filter, int out_channels, unsigned char* out,
                 float* logits, hipStream_t s) {
    CTRL_CHECK(maps4 && par5 && out, "pidi_fuse: null pointer");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "pidi_fuse: out_channels must be 1 or 3");
    TRY(check_map("pidi_fuse", N, H, W, 3));
    CTRL_CHECK(H % 8 == 0 && W % 8 == 0, "pidi_fuse: H and W must be multiples of 8 (the four maps have strides 1 .. 8)");
    CTRL_CHECK(((uintptr_t)out & 3) == 0, "pidi_fuse: out must be 4-byte aligned");
    FusePar m;
    for (int k = 0; k < 4; ++k) {
        CTRL_CHECK(maps4[k] != nullptr, "pidi_fuse: null map");
        m.p[k] = maps4[k];
        m.w[k] = par5[k];
    }
    m.b = par5[4];
    const long quads = (long)N * H * W / 4;
    const dim3 grid((unsigned)((quads + NT - 1) / NT));
    PROF_WORK(0, (double)N * H * W * (4.0 * 1.33 + out_channels + (logits ? 4 : 0)));
    prof_detail("N%d %dx%d ch%d", N, H, W, out_channels);
    if (out_channels == 3) LAUNCH("pidi", pidi_fuse_kernel<3>, grid, dim3(NT), 0, s, m, H, W, quads, apply_filter ? 1 : 0, out, logits);
    else LAUNCH("pidi", pidi_fuse_kernel<1>, grid, dim3(NT), 0, s, m, H, W, quads, apply_filter ? 1 : 0, out, logits);
    return 0;
}
