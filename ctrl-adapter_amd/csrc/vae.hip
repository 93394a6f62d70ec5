// KL-VAE encoder kernels (diffusers AutoencoderKL / AutoencoderKLTemporalDecoder encoder half: the image latents of the SVD pipeline's
// _encode_vae_image and I2VGen-XL's prepare_image_latents; csrc/plan_vae.cpp chains them with the implicit GEMM and the GroupNorm):
//   vae_row_softmax_kernel  the mid-block attention's softmax (one head of dim 512 over L = h * w tokens, past the flash kernels'
//                           head_dim): S = Q K^T / sqrt(D) rows in fp32 (the GEMM's output) -> P fp16, max / exp / sum in fp32 as
//                           diffusers' upcast_softmax; pad columns up to Lpad zeroed (they are the K axis of the P V GEMM)
//   vae_conv_in_kernel      conv_in (3 -> C0, 3x3, padding 1) on the NCHW pixels of any dtype, in fp32 into the fp32 residual stream:
//                           the fp16 output of the shared direct kernel (smallconv.hip) alone put 6e-4 on the latents
//   vae_posterior_kernel    conv_out rows -> quant_conv (1x1, fp32) -> DiagonalGaussianDistribution: mean | logvar clamped to
//                           [-30, 20], std = exp(logvar / 2), var = exp(logvar) -> mode / sample / moments, NCHW
// and of the decoder half (AutoencoderKL.decode; csrc/plan_vae_decoder.cpp):
//   vae_dec_head_kernel     latents * scale -> post_quant_conv -> conv_in, all fp32, NCHW latents of any dtype -> the fp32 NHWC stream
//   vae_dec_tail_kernel     conv_norm_out + SiLU + conv_out + the output epilogue (sample / [0, 1] / uint8) in one pass over the stream
// and of the temporal decoder (AutoencoderKLTemporalDecoder.decode; csrc/plan_vae_tdecoder.cpp):
//   vae_time_conv_kernel    time_conv_out over the frames of a clip (the tail kernel's fp32 samples) + the same output epilogue
// Each computes a row or a pixel on its own: an image's results do not depend on the batch it is in.
#include "ops.h"
#include <math.h>

namespace {

constexpr int kSmThreads = 256;

__device__ __forceinline__ float block_reduce256(float v, float* red, bool is_max) {
    v = is_max ? wave_max(v) : wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per row: three coalesced passes over the fp32 scores (max, sum of exp, normalised write); the row (<= 64 KB at
// L = 16384) stays in L2 between the passes
__global__ void __launch_bounds__(kSmThreads) vae_row_softmax_kernel(const float* __restrict__ S, long lds, half_t* __restrict__ P, long ldp,
                                                                      int L, int Lpad) {
    __shared__ float red[4];
    const float* s = S + (size_t)blockIdx.x * lds;
    half_t* p = P + (size_t)blockIdx.x * ldp;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < L; c += kSmThreads) m = fmaxf(m, s[c]);
    m = block_reduce256(m, red, true);
    float z = 0.f;
    for (int c = threadIdx.x; c < L; c += kSmThreads) z += expf(s[c] - m);
    z = block_reduce256(z, red, false);
    const float rz = 1.0f / z;
    for (int c = threadIdx.x; c < L; c += kSmThreads) p[c] = (half_t)(expf(s[c] - m) * rz);
    for (int c = L + threadIdx.x; c < Lpad; c += kSmThreads) p[c] = (half_t)0.f;
}

// one thread per (pixel, 16 output channels): the 27 taps in registers, out[pix][c] = b[c] + sum w[tap][ci][c] * x (zero outside the map)
__global__ void __launch_bounds__(256) vae_conv_in_kernel(const void* __restrict__ px, int dt, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ out, int H, int W, int Cout) {
    const int groups = Cout / 16;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W * groups) return;
    const int pix = (int)(i / groups), c0 = (int)(i - (long)pix * groups) * 16;
    const int y = pix / W, x = pix - y * W;
    float v[27];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) v[t * 3 + ci] = ok ? load_as_f32(px, ((size_t)ci * H + yy) * W + xx, dt) : 0.f;
    }
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = b[c0 + c];
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(w[(size_t)k * Cout + c0 + c], v[k], acc[c]);
    float4* o = (float4*)(out + (size_t)pix * Cout + c0);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
}

constexpr int kMaxLat = 8;

// one thread per latent pixel (n, y, x)
__global__ void __launch_bounds__(256) vae_posterior_kernel(const float* __restrict__ x, long ldx, int x_nchw, const float* __restrict__ wq,
                                                            const float* __restrict__ bq, int N, int lat, int hw, const void* __restrict__ eps,
                                                            int eps_dt, float scale, int kind, void* __restrict__ out, int out_dt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * hw) return;
    const int n = (int)(i / hw), pix = (int)(i - (long)n * hw);
    const int C2 = 2 * lat;
    float v[2 * kMaxLat], q[2 * kMaxLat];
#pragma unroll
    for (int c = 0; c < 2 * kMaxLat; ++c)
        v[c] = c < C2 ? (x_nchw ? x[((size_t)n * ldx + c) * hw + pix] : x[(size_t)i * ldx + c]) : 0.f;
#pragma unroll
    for (int o = 0; o < 2 * kMaxLat; ++o) {
        if (!wq) { q[o] = v[o]; continue; }
        float a = 0.f;
        if (o < C2) {
            a = bq ? bq[o] : 0.f;
#pragma unroll
            for (int c = 0; c < 2 * kMaxLat; ++c)
                if (c < C2) a = fmaf(wq[o * C2 + c], v[c], a);
        }
        q[o] = a;
    }
#pragma unroll
    for (int c = 0; c < kMaxLat; ++c) {
        if (c >= lat) break;
        const float mean = q[c];
        const float logvar = fminf(fmaxf(q[lat + c], -30.0f), 20.0f);
        const size_t o = ((size_t)n * lat + c) * hw + pix;
        if (kind == CTRL_VAE_MOMENTS) {
            const size_t b = (size_t)n * 4 * lat * hw + pix;
            store_from_f32(out, b + (size_t)c * hw, out_dt, mean);
            store_from_f32(out, b + (size_t)(lat + c) * hw, out_dt, logvar);
            store_from_f32(out, b + (size_t)(2 * lat + c) * hw, out_dt, expf(0.5f * logvar));
            store_from_f32(out, b + (size_t)(3 * lat + c) * hw, out_dt, expf(logvar));
        } else if (kind == CTRL_VAE_SAMPLE) {
            const float e = load_as_f32(eps, o, eps_dt);
            store_from_f32(out, o, out_dt, fmaf(expf(0.5f * logvar), e, mean) * scale);
        } else {
            store_from_f32(out, o, out_dt, mean * scale);
        }
    }
}

// decoder head, one thread per (latent pixel, 16 output channels): for each of the 9 taps the lat latents of the tapped pixel * scale go
// through post_quant_conv (fp32), zero outside the map (conv_in pads ITS input, the post_quant_conv result), then into the 16 sums.
// cs: elements between the channel planes of z (H * W when dense; a frame of a [C][F][h][w] clip has F * h * w)
__global__ void __launch_bounds__(256) vae_dec_head_kernel(const void* __restrict__ z, int dt, float scale, const float* __restrict__ wpq,
                                                           const float* __restrict__ bpq, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ out, int lat, int H, int W,
                                                           long cs, int Cout) {
    const int groups = Cout / 16;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W * groups) return;
    const int pix = (int)(i / groups), c0 = (int)(i - (long)pix * groups) * 16;
    const int y = pix / W, x = pix - y * W;
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = b[c0 + c];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        float v[kMaxLat];
#pragma unroll
        for (int ci = 0; ci < kMaxLat; ++ci) v[ci] = ci < lat ? load_as_f32(z, (size_t)ci * cs + (size_t)yy * W + xx, dt) * scale : 0.f;
#pragma unroll
        for (int o = 0; o < kMaxLat; ++o) {
            if (o >= lat) break;
            float q = bpq[o];
#pragma unroll
            for (int ci = 0; ci < kMaxLat; ++ci)
                if (ci < lat) q = fmaf(wpq[o * lat + ci], v[ci], q);
            const float* wr = w + ((size_t)t * lat + o) * Cout + c0;
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fmaf(wr[c], q, acc[c]);
        }
    }
    float4* o4 = (float4*)(out + (size_t)pix * Cout + c0);
#pragma unroll
    for (int c = 0; c < 4; ++c) o4[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
}

// decoder tail: conv_norm_out + SiLU + conv_out (C -> COUT <= 4, 3x3) + the output epilogue in ONE pass over the fp32 stream.  A
// workgroup owns a kTailW x kTailH tile of output pixels (one per thread) and walks the channels in chunks of kTailCk: the chunk's halo
// patch is staged in LDS already normalised and activated (zero outside the map: the convolution pads the ACTIVATED map), then every
// thread adds its 9 taps x kTailCk channels into COUT fp32 sums; the weights are uniform across the workgroup (scalar loads).
constexpr int kTailW = 32, kTailH = 8, kTailCk = 32;
constexpr int kTailPs = kTailCk + 4;                                  // floats between the pixels of the patch (16-byte aligned, off the bank stride)
constexpr int kTailPw = kTailW + 2, kTailPix = (kTailH + 2) * kTailPw;

__device__ __forceinline__ float round_to_dt(float v, int dt) {
    if (dt == DT_F16) return (float)(half_t)v;
    if (dt == DT_BF16) return bf16_to_f32(f32_to_bf16(v));
    return v;
}

template <int COUT>
__global__ void __launch_bounds__(256) vae_dec_tail_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ w, const float* __restrict__ b, int H, int W, int C,
                                                           int kind, void* __restrict__ out, int out_dt) {
    __shared__ __attribute__((aligned(16))) float patch[kTailPix * kTailPs];
    __shared__ float sc[kTailCk], sf[kTailCk];     // the chunk's rstd * gamma and beta - mean * rstd * gamma
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTailW, y0 = blockIdx.y * kTailH;
    const int cg = C / 32;
    const float inv_cnt = 1.0f / ((float)H * (float)W * (float)cg);
    const int lx = tid & (kTailW - 1), ly = tid / kTailW;
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
    for (int c0 = 0; c0 < C; c0 += kTailCk) {
        __syncthreads();                           // the previous chunk's patch and scales have been read
        if (tid < kTailCk) {                       // the arithmetic of gn_apply_kernel (norm.hip)
            const int c = c0 + tid, g = c / cg;
            const float s = stats[g * 2], ss = stats[g * 2 + 1];
            const float mean = s * inv_cnt;
            const float var = fmaxf(ss * inv_cnt - mean * mean, 0.f);
            const float rstd = rsqrtf(var + eps);
            sc[tid] = rstd * gamma[c];
            sf[tid] = beta[c] - mean * sc[tid];
        }
        __syncthreads();
        for (int it = tid; it < kTailPix * (kTailCk / 4); it += 256) {
            const int p = it / (kTailCk / 4), q = it - p * (kTailCk / 4);
            const int py = p / kTailPw, px = p - py * kTailPw;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int c = q * 4;
                const float4 r = *(const float4*)(x + ((size_t)gy * W + gx) * C + c0 + c);
                v.x = silu_f(fmaf(r.x, sc[c], sf[c]));
                v.y = silu_f(fmaf(r.y, sc[c + 1], sf[c + 1]));
                v.z = silu_f(fmaf(r.z, sc[c + 2], sf[c + 2]));
                v.w = silu_f(fmaf(r.w, sc[c + 3], sf[c + 3]));
            }
            *(float4*)(patch + p * kTailPs + q * 4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float* pp = patch + ((ly + t / 3) * kTailPw + lx + t % 3) * kTailPs;
            const float* wt = w + ((size_t)t * C + c0) * COUT;
#pragma unroll
            for (int q = 0; q < kTailCk / 4; ++q) {
                const float4 v = *(const float4*)(pp + q * 4);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < COUT; ++o) acc[o] = fmaf(wt[(q * 4 + j) * COUT + o], vv[j], acc[o]);
            }
        }
    }
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) return;
    const size_t hw = (size_t)H * W, pix = (size_t)gy * W + gx;
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        const float v = round_to_dt(acc[o] + b[o], out_dt);       // what .sample holds in the module's dtype
        if (kind == CTRL_VAE_DEC_SAMPLE) {
            store_from_f32(out, (size_t)o * hw + pix, out_dt, v);
        } else {
            const float u = fminf(fmaxf(v * 0.5f + 0.5f, 0.f), 1.f);
            if (kind == CTRL_VAE_DEC_UNIT) ((float*)out)[(size_t)o * hw + pix] = u;
            else ((unsigned char*)out)[pix * COUT + o] = (unsigned char)rintf(u * 255.0f);      // rintf: ties to even, as numpy's round
        }
    }
}

// time_conv_out of the temporal decoder (Conv3d (3,1,1), padding (1,0,0), OC -> OC) over the fp32 NCHW frames x [F][OC][HW] the tail
// kernel wrote, + the output epilogue.  Memory-bound: a thread owns all OC channels of PV consecutive pixels (VEC: 4, one 16-byte load
// per plane; consecutive lanes read consecutive 16 bytes) and walks kTcFrames frames with a three-frame window in registers, so a plane
// is read once per walk (+ its two halo frames); the 3 * OC * OC weights are uniform (scalar loads).  Frames outside [0, F) are zero.
constexpr int kTcFrames = 4;

template <int OC, bool VEC>
__global__ void __launch_bounds__(256) vae_time_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, int F, long HW, int kind, void* __restrict__ out,
                                                            int out_dt) {
    constexpr int PV = VEC ? 4 : 1;
    const size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * PV;
    if (p0 >= (size_t)HW) return;
    const int f0 = blockIdx.y * kTcFrames, f1 = min(F, f0 + kTcFrames);
    float win[3][OC][PV];                          // frames f - 1, f, f + 1
    auto load = [&](int f, float (&dst)[OC][PV]) {
#pragma unroll
        for (int c = 0; c < OC; ++c) {
            if (f < 0 || f >= F) {
#pragma unroll
                for (int j = 0; j < PV; ++j) dst[c][j] = 0.f;
            } else {
                const float* p = x + ((size_t)f * OC + c) * (size_t)HW + p0;
                if (VEC) {
                    const f4 v = *(const f4*)p;
#pragma unroll
                    for (int j = 0; j < PV; ++j) dst[c][j] = v[j];
                } else {
                    dst[c][0] = *p;
                }
            }
        }
    };
    load(f0 - 1, win[0]);
    load(f0, win[1]);
    for (int f = f0; f < f1; ++f) {
        load(f + 1, win[2]);
        float y[OC][PV];
#pragma unroll
        for (int o = 0; o < OC; ++o) {
#pragma unroll
            for (int j = 0; j < PV; ++j) {
                float acc = b[o];
#pragma unroll
                for (int c = 0; c < OC; ++c)
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc = fmaf(w[(o * OC + c) * 3 + t], win[t][c][j], acc);
                y[o][j] = round_to_dt(acc, out_dt);       // what .sample holds in the module's dtype
            }
        }
        if (kind == CTRL_VAE_DEC_U8) {
            // NHWC bytes: the thread's PV pixels x OC channels are PV * OC consecutive bytes (VEC: OC aligned 32-bit words)
            unsigned char q[PV * OC];
#pragma unroll
            for (int j = 0; j < PV; ++j)
#pragma unroll
                for (int o = 0; o < OC; ++o)
                    q[j * OC + o] = (unsigned char)rintf(fminf(fmaxf(y[o][j] * 0.5f + 0.5f, 0.f), 1.f) * 255.0f);      // ties to even
            unsigned char* op = (unsigned char*)out + ((size_t)f * (size_t)HW + p0) * OC;
            if (VEC) {
#pragma unroll
                for (int k = 0; k < OC; ++k)
                    ((unsigned*)op)[k] = (unsigned)q[4 * k] | ((unsigned)q[4 * k + 1] << 8) | ((unsigned)q[4 * k + 2] << 16) | ((unsigned)q[4 * k + 3] << 24);
            } else {
#pragma unroll
                for (int o = 0; o < OC; ++o) op[o] = q[o];
            }
        } else {
            const bool unit = kind == CTRL_VAE_DEC_UNIT;
#pragma unroll
            for (int o = 0; o < OC; ++o) {
                const size_t i = ((size_t)f * OC + o) * (size_t)HW + p0;
                float v[PV];
#pragma unroll
                for (int j = 0; j < PV; ++j) v[j] = unit ? fminf(fmaxf(y[o][j] * 0.5f + 0.5f, 0.f), 1.f) : y[o][j];
                if (!VEC) {
                    if (unit) ((float*)out)[i] = v[0];
                    else store_from_f32(out, i, out_dt, v[0]);
                } else if (unit || out_dt == DT_F32) {
                    *(f4*)((float*)out + i) = f4{v[0], v[1], v[2], v[3]};
                } else if (out_dt == DT_F16) {
                    *(h4*)((half_t*)out + i) = h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                } else {
                    typedef u16 us4 __attribute__((ext_vector_type(4)));
                    *(us4*)((u16*)out + i) = us4{f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
                }
            }
        }
#pragma unroll
        for (int c = 0; c < OC; ++c)
#pragma unroll
            for (int j = 0; j < PV; ++j) { win[0][c][j] = win[1][c][j]; win[1][c][j] = win[2][c][j]; }
    }
}

template <int OC>
int launch_time_conv(bool vec, dim3 grid, hipStream_t s, const float* x, const float* w, const float* b, int F, long HW, int kind, void* out,
                     int out_dt) {
    if (vec) LAUNCH("vae_time_conv", (vae_time_conv_kernel<OC, true>), grid, dim3(256), 0, s, x, w, b, F, HW, kind, out, out_dt);
    else LAUNCH("vae_time_conv", (vae_time_conv_kernel<OC, false>), grid, dim3(256), 0, s, x, w, b, F, HW, kind, out, out_dt);
    return 0;
}

}  // namespace

int op_vae_time_conv(const float* x, const float* w, const float* b, int F, int H, int W, int Cout, int kind, void* out, int out_dt,
                     hipStream_t s) {
    CTRL_CHECK(x && w && b && out, "vae_time_conv: null argument");
    CTRL_CHECK(F >= 1 && H >= 1 && W >= 1 && Cout >= 1 && Cout <= 4, "vae_time_conv: bad shape (1 <= channels <= 4)");
    CTRL_CHECK(kind == CTRL_VAE_DEC_SAMPLE || kind == CTRL_VAE_DEC_UNIT || kind == CTRL_VAE_DEC_U8,
               "vae_time_conv: kind must be 0 sample, 1 unit or 2 u8");
    CTRL_CHECK(out_dt >= DT_F32 && out_dt <= DT_BF16, "vae_time_conv: bad dtype");
    const long HW = (long)H * W;
    // 16-byte loads and the packed stores need whole groups of 4 pixels per plane and aligned bases
    // (4 output pixels are 16 bytes of fp32, 8 of fp16 / bf16, or Cout 32-bit words of NHWC bytes)
    const uintptr_t oalign = kind == CTRL_VAE_DEC_U8 ? 3 : ((kind == CTRL_VAE_DEC_UNIT || out_dt == DT_F32) ? 15 : 7);
    const bool vec = HW % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & oalign) == 0;
    const long threads = vec ? HW / 4 : HW;
    const long gx = (threads + 255) / 256, gy = (F + kTcFrames - 1) / kTcFrames;
    CTRL_CHECK(gx < (1L << 31) && gy <= 65535, "vae_time_conv: too large");
    const dim3 grid((unsigned)gx, (unsigned)gy);
    const double osz = kind == CTRL_VAE_DEC_SAMPLE ? (out_dt == DT_F32 ? 4.0 : 2.0) : (kind == CTRL_VAE_DEC_UNIT ? 4.0 : 1.0);
    PROF_WORK(2.0 * 3 * Cout * Cout * F * (double)HW, (double)F * HW * Cout * (4.0 + osz));
    switch (Cout) {
        case 1: return launch_time_conv<1>(vec, grid, s, x, w, b, F, HW, kind, out, out_dt);
        case 2: return launch_time_conv<2>(vec, grid, s, x, w, b, F, HW, kind, out, out_dt);
        case 3: return launch_time_conv<3>(vec, grid, s, x, w, b, F, HW, kind, out, out_dt);
        default: return launch_time_conv<4>(vec, grid, s, x, w, b, F, HW, kind, out, out_dt);
    }
}

int op_vae_row_softmax(const float* S, long lds, half_t* P, long ldp, int rows, int L, int Lpad, hipStream_t s) {
    CTRL_CHECK(S && P, "vae_row_softmax: null argument");
    CTRL_CHECK(rows >= 1 && L >= 1 && Lpad >= L && lds >= L && ldp >= Lpad, "vae_row_softmax: bad shape");
    PROF_WORK(4.0 * rows * L, (double)rows * (L * 4.0 * 3.0 + Lpad * 2.0));
    LAUNCH("vae_softmax", vae_row_softmax_kernel, dim3(rows), dim3(kSmThreads), 0, s, S, lds, P, ldp, L, Lpad);
    return 0;
}

int op_vae_conv_in(const void* px, int dt, const float* w, const float* b, float* out, int H, int W, int Cout, hipStream_t s) {
    CTRL_CHECK(px && w && b && out, "vae_conv_in: null argument");
    CTRL_CHECK(H >= 1 && W >= 1 && Cout >= 16 && Cout % 16 == 0 && dt >= DT_F32 && dt <= DT_BF16 && ((uintptr_t)out & 15) == 0,
               "vae_conv_in: bad shape (Cout % 16 == 0), dtype or alignment");
    const long n = (long)H * W * (Cout / 16);
    PROF_WORK(2.0 * 27 * H * W * Cout, (double)H * W * (3 * 4.0 + Cout * 4.0));
    LAUNCH("vae_conv_in", vae_conv_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, px, dt, w, b, out, H, W, Cout);
    return 0;
}

int op_vae_posterior(const float* x, long ldx, int x_nchw, const float* wq, const float* bq, int N, int lat, int h, int w, const void* eps,
                     int eps_dt, float scale, int kind, void* out, int out_dt, hipStream_t s) {
    CTRL_CHECK(x && out, "vae_posterior: null argument");
    CTRL_CHECK(N >= 1 && lat >= 1 && lat <= kMaxLat && h >= 1 && w >= 1 && ldx >= 2 * lat, "vae_posterior: bad shape (1 <= latent channels <= 8)");
    CTRL_CHECK(kind == CTRL_VAE_MODE || kind == CTRL_VAE_SAMPLE || kind == CTRL_VAE_MOMENTS, "vae_posterior: kind must be 0 mode, 1 sample or 2 moments");
    CTRL_CHECK(kind != CTRL_VAE_SAMPLE || eps != nullptr, "vae_posterior: sampling needs eps");
    CTRL_CHECK(out_dt >= DT_F32 && out_dt <= DT_BF16 && (kind != CTRL_VAE_SAMPLE || (eps_dt >= DT_F32 && eps_dt <= DT_BF16)),
               "vae_posterior: bad dtype");
    const long n = (long)N * h * w;
    CTRL_CHECK(n * 4 * lat < (1L << 31) * 2, "vae_posterior: too large");
    PROF_WORK((double)n * (2.0 * 4 * lat * lat + 8.0 * lat), (double)n * (2 * lat * 4.0 + lat * (kind == CTRL_VAE_MOMENTS ? 16.0 : 4.0)));
    LAUNCH("vae_posterior", vae_posterior_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, ldx, x_nchw, wq, bq, N, lat, h * w,
           eps, eps_dt, scale, kind, out, out_dt);
    return 0;
}

int op_vae_dec_head(const void* z, int dt, float scale, const float* wpq, const float* bpq, const float* w, const float* b, float* out,
                    int lat, int h, int wd, long ch_stride, int Cout, hipStream_t s) {
    CTRL_CHECK(z && wpq && bpq && w && b && out, "vae_dec_head: null argument");
    CTRL_CHECK(lat >= 1 && lat <= kMaxLat && h >= 1 && wd >= 1 && Cout >= 16 && Cout % 16 == 0 && dt >= DT_F32 && dt <= DT_BF16 &&
                   ((uintptr_t)out & 15) == 0,
               "vae_dec_head: bad shape (1 <= latent channels <= 8, Cout % 16 == 0), dtype or alignment");
    CTRL_CHECK(ch_stride >= (long)h * wd, "vae_dec_head: the channel stride must be at least h * w elements");
    const long n = (long)h * wd * (Cout / 16);
    CTRL_CHECK(n < (1L << 31), "vae_dec_head: too large");
    PROF_WORK(2.0 * h * wd * (9.0 * lat * lat * (Cout / 16) + 9.0 * lat * Cout), (double)h * wd * (lat * 4.0 + Cout * 4.0));
    LAUNCH("vae_dec_head", vae_dec_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, dt, scale, wpq, bpq, w, b, out, lat,
           h, wd, ch_stride, Cout);
    return 0;
}

int op_vae_dec_tail(const float* x, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b,
                    int H, int W, int C, int Cout, int kind, void* out, int out_dt, hipStream_t s) {
    CTRL_CHECK(x && stats && gamma && beta && w && b && out, "vae_dec_tail: null argument");
    CTRL_CHECK(H >= 1 && W >= 1 && H <= 65535 * kTailH && W <= 65535 * kTailW && C >= 32 && C <= 2048 && C % 32 == 0 && Cout >= 1 && Cout <= 4 &&
                   ((uintptr_t)x & 15) == 0,
               "vae_dec_tail: bad shape (C a multiple of 32 up to 2048, 1 <= Cout <= 4) or alignment");
    CTRL_CHECK(kind == CTRL_VAE_DEC_SAMPLE || kind == CTRL_VAE_DEC_UNIT || kind == CTRL_VAE_DEC_U8,
               "vae_dec_tail: kind must be 0 sample, 1 unit or 2 u8");
    CTRL_CHECK(out_dt >= DT_F32 && out_dt <= DT_BF16, "vae_dec_tail: bad dtype");
    const dim3 grid((unsigned)((W + kTailW - 1) / kTailW), (unsigned)((H + kTailH - 1) / kTailH));
    PROF_WORK(2.0 * 9 * H * W * (double)C * Cout, (double)H * W * (C * 4.0 + Cout * 4.0));
    switch (Cout) {
        case 1: LAUNCH("vae_dec_tail", vae_dec_tail_kernel<1>, grid, dim3(256), 0, s, x, stats, gamma, beta, eps, w, b, H, W, C, kind, out, out_dt); break;
        case 2: LAUNCH("vae_dec_tail", vae_dec_tail_kernel<2>, grid, dim3(256), 0, s, x, stats, gamma, beta, eps, w, b, H, W, C, kind, out, out_dt); break;
        case 3: LAUNCH("vae_dec_tail", vae_dec_tail_kernel<3>, grid, dim3(256), 0, s, x, stats, gamma, beta, eps, w, b, H, W, C, kind, out, out_dt); break;
        default: LAUNCH("vae_dec_tail", vae_dec_tail_kernel<4>, grid, dim3(256), 0, s, x, stats, gamma, beta, eps, w, b, H, W, C, kind, out, out_dt); break;
    }
    return 0;
}
