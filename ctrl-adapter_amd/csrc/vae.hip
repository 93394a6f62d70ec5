// KL-VAE encoder kernels (diffusers AutoencoderKL / AutoencoderKLTemporalDecoder encoder half: the image latents of the SVD pipeline's
// _encode_vae_image and I2VGen-XL's prepare_image_latents; csrc/plan_vae.cpp chains them with the implicit GEMM and the GroupNorm):
//   vae_row_softmax_kernel  the mid-block attention's softmax (one head of dim 512 over L = h * w tokens, past the flash kernels'
//                           head_dim): S = Q K^T / sqrt(D) rows in fp32 (the GEMM's output) -> P fp16, max / exp / sum in fp32 as
//                           diffusers' upcast_softmax; pad columns up to Lpad zeroed (they are the K axis of the P V GEMM)
//   vae_conv_in_kernel      conv_in (3 -> C0, 3x3, padding 1) on the NCHW pixels of any dtype, in fp32 into the fp32 residual stream:
//                           the fp16 output of the shared direct kernel (smallconv.hip) alone put 6e-4 on the latents
//   vae_posterior_kernel    conv_out rows -> quant_conv (1x1, fp32) -> DiagonalGaussianDistribution: mean | logvar clamped to
//                           [-30, 20], std = exp(logvar / 2), var = exp(logvar) -> mode / sample / moments, NCHW
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

}  // namespace

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
