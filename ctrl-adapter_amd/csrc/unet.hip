// Kernels of the backbone UNets (SVD: plan_unet_st.cpp, SDXL: plan_unet2d.cpp, I2VGen-XL: plan_unet_i2v.cpp; gfx950) that no other plan has:
//   unet_skip_join_kernel   one skip tensor of the up path: fp32 NHWC skip (+ the adapter's residual, read in the caller's NCHW / NCFHW
//                           layout) -> columns [col, col + C2) of the up ResNet's concatenated operand, fp32 master + fp16 mirror
//   unet_conv_out_kernel    conv_out 3x3, C0 -> <= 4 channels, on the normalised + activated fp16 map -> NCHW in the sample's dtype
//   unet_text_time_kernel   SDXL's text_time addition embedding: the operand rows of add_embedding.linear_1, [text_embeds | sinusoids of
//                           the time ids], in one launch (a few KB: latency only)
//   i2v_frames_kernel       I2VGen-XL's image_latents b c f h w -> fp32 planes (b f) c h w, the small stems' input
//   i2v_latent_encoder_kernel   I2VGenXLTransformerTemporalEncoder (dim 4) over the frames of every pixel + the conv_in operand rows
//   adaptive_avgpool_nhwc_kernel   AdaptiveAvgPool2d to a fixed OH x OW with floor / ceil windows, channels-last
// The first two are HBM-bound: the join moves 4 (skip) + 2..4 (residual) + 6 (master + mirror) bytes per element once; conv_out reads the C0-wide
// map (its nine taps overlap in L1 / L2) and writes 4 channels.
#include "ops.h"

namespace {

// grid (ceil(HW / 64), C2 / 32, B * F).  The residual tile [32 c][64 p] is read along the pixels (its NCHW planes are dense in p) and
// transposed through LDS, as nchw_to_nhwc_kernel does; then a thread owns 8 consecutive channels of one pixel: two 16-byte fp32 loads
// of the skip, one fp32 add, two 16-byte fp32 stores and one 16-byte fp16 store.  skip / out32 may be the same buffer (the mid
// residual is added in place): every element is read and written by the same thread.
__global__ __launch_bounds__(256) void unet_skip_join_kernel(const float* skip, long ld_skip, const void* __restrict__ res, int res_dt,
                                                             long res_frame_b, long res_frame_f, long res_ch, int F, int HW, int C2,
                                                             float* out32, half_t* out16, long ld_out, int col, int lo_off) {
    __shared__ float tile[32][65];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 64;
    const int t = threadIdx.x;
    if (res) {
        const size_t base = (size_t)(n / F) * res_frame_b + (size_t)(n % F) * res_frame_f;
        const int pl = t & 63, p = p0 + pl;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = (t >> 6) + 4 * i;
            tile[cl][pl] = p < HW ? load_as_f32(res, base + (size_t)(c0 + cl) * res_ch + p, res_dt) : 0.f;
        }
        __syncthreads();
    }
    const int pl = t >> 2, cq = (t & 3) * 8, p = p0 + pl;
    if (p >= HW) return;
    const size_t row = (size_t)n * HW + p;
    const float* sp = skip + row * ld_skip + c0 + cq;
    const f4 a = *(const f4*)sp, b = *(const f4*)(sp + 4);
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    if (res) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += tile[cq + j][pl];
    }
    const size_t o = row * ld_out + col + c0 + cq;
    *(f4*)(out32 + o) = f4{v[0], v[1], v[2], v[3]};
    *(f4*)(out32 + o + 4) = f4{v[4], v[5], v[6], v[7]};
    if (out16) {
        h8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
        if (!lo_off) {
            *(h8*)(out16 + o) = h;
        } else {      // split mirror: rows 2 * ld_out wide, the rounding residual rides along (hi + lo == x to ~2^-22)
            h8 l;
#pragma unroll
            for (int j = 0; j < 8; ++j) l[j] = (half_t)(v[j] - (float)h[j]);
            const size_t o2 = row * 2 * ld_out + col + c0 + cq;
            *(h8*)(out16 + o2) = h;
            *(h8*)(out16 + o2 + lo_off) = l;
        }
    }
}

// 64 output pixels per workgroup, four lanes per pixel: lane q of a pixel walks the 8-channel chunks q, q + 4, ... of every tap (the
// four lanes read 64 consecutive bytes), the partial sums meet through two lane exchanges.  w fp32 [9][C][Cout] (op_pack_conv_w_direct).
__global__ __launch_bounds__(256) void unet_conv_out_kernel(const half_t* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, void* __restrict__ out, int out_dt, int N,
                                                            int H, int W, int C, int Cout, int F, long s_b, long s_f, long s_c, long s_p) {
    const int t = threadIdx.x, q = t & 3;
    const size_t npix = (size_t)N * H * W;
    const size_t pix = (size_t)blockIdx.x * 64 + (t >> 2);
    const bool live = pix < npix;
    const size_t pc = live ? pix : 0;
    const int ox = (int)(pc % W);
    const size_t r = pc / W;
    const int oy = (int)(r % H);
    const int n = (int)(r / H);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        if (!live || iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const half_t* ip = x + (((size_t)n * H + iy) * W + ix) * C;
        const float* wt = w + (size_t)tap * C * Cout;
        for (int c = q * 8; c < C; c += 32) {
            const h8 v = *(const h8*)(ip + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xv = (float)v[j];
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < Cout) acc[o] = fmaf(wt[(size_t)(c + j) * Cout + o], xv, acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        acc[o] += __shfl_xor(acc[o], 1, 64);
        acc[o] += __shfl_xor(acc[o], 2, 64);
    }
    if (!live || q != 0) return;
    // image n = (b, f) of F frames per clip lands at b * s_b + f * s_f, its channel o at + o * s_c, its pixel p at + p * s_p
    const size_t p = (size_t)oy * W + ox;
    const size_t base = (size_t)(n / F) * s_b + (size_t)(n % F) * s_f + p * s_p;
    for (int o = 0; o < Cout; ++o) store_from_f32(out, base + (size_t)o * s_c, out_dt, acc[o] + bias[o]);
}

// image_latents [B][4][F][HW] (any dtype) -> fp32 planes [(b f)][4][HW]: what the direct convolutions of the two latent stems read
__global__ __launch_bounds__(256) void i2v_frames_kernel(const void* __restrict__ x, int dt, float* __restrict__ y, int F, int HW, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t p = i % HW, r = i / HW;
    const int c = (int)(r % 4);
    const size_t bf = r / 4;
    const size_t b = bf / F, f = bf % F;
    y[i] = load_as_f32(x, ((b * 4 + c) * F + f) * HW + p, dt);
}

// I2VGenXLTransformerTemporalEncoder with dim 4 (two heads of 4, feed-forward 4 -> 16 -> 4, erf GELU, softmax scale 0.5) over the F
// frames of every pixel, fp32 throughout.  One lane per (pixel, frame): a workgroup holds P = 256 / F pixels, lane t is frame t / P of
// pixel t % P, so the lanes of a frame read and write consecutive pixels (16 bytes each: the loads and stores of a wave are dense).
// Every lane normalises its token and projects q, k, v (4 -> 8); k and v meet through LDS as four 16-byte chunks per token, chunk-major
// (consecutive lanes 16 bytes apart: no bank conflicts); then the lane walks the F keys of its pixel twice (maximum, then exp and
// the weighted sum), applies to_out, the residual, the feed-forward and its residual.  The 288 weight scalars sit in LDS.
// wts: ln g[4] b[4] | to_q [8][4] | to_k [8][4] | to_v [8][4] | to_out [4][8] b[4] | ff1 [16][4] b[16] | ff2 [4][16] b[4]
// out8 rows [(b f) HW][8]: columns 4..7 = the encoded latents, columns 0..3 = the sample (b c f h w, any dtype) converted once;
// keep (optional) [(b f) HW][4]: the encoded latents once more, for the step-invariant cache.  precomputed: x already holds the
// encoded latents (a kept forward's `keep`): they are copied.
constexpr int kI2vEncWts = 288;
__global__ __launch_bounds__(256) void i2v_latent_encoder_kernel(const float* __restrict__ x, const float* __restrict__ wts,
                                                                 const void* __restrict__ sample, int sample_dt, float* __restrict__ out8,
                                                                 float* __restrict__ keep, int B, int F, int HW, int P, int precomputed) {
    __shared__ float w[kI2vEncWts];
    __shared__ f4 kv[4][256];
    const int t = threadIdx.x;
    if (!precomputed) {
        for (int i = t; i < kI2vEncWts; i += 256) w[i] = wts[i];
    }
    const int f = t / P, pl = t - f * P;
    const size_t gp = (size_t)blockIdx.x * P + pl;
    const bool live = f < F && gp < (size_t)B * HW;
    const size_t b = live ? gp / HW : 0, p = live ? gp % HW : 0;
    const size_t row = (b * F + (live ? f : 0)) * HW + p;
    f4 xv = live ? *(const f4*)(x + row * 4) : f4{0.f, 0.f, 0.f, 0.f};
    f4 res = xv;
    if (!precomputed) {
        __syncthreads();
        // LayerNorm(4), eps 1e-5, two-pass statistics
        const float mean = ((xv[0] + xv[1]) + (xv[2] + xv[3])) * 0.25f;
        const float d0 = xv[0] - mean, d1 = xv[1] - mean, d2 = xv[2] - mean, d3 = xv[3] - mean;
        const float var = ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * 0.25f;
        const float rstd = 1.0f / sqrtf(var + 1e-5f);
        const float xn[4] = {d0 * rstd * w[0] + w[4], d1 * rstd * w[1] + w[5], d2 * rstd * w[2] + w[6], d3 * rstd * w[3] + w[7]};
        float q[8], k[8], v[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float aq = 0.f, ak = 0.f, av = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                aq = fmaf(xn[c], w[8 + o * 4 + c], aq);
                ak = fmaf(xn[c], w[40 + o * 4 + c], ak);
                av = fmaf(xn[c], w[72 + o * 4 + c], av);
            }
            q[o] = aq; k[o] = ak; v[o] = av;
        }
        if (f < F) {           // (lanes of a pixel beyond the batch still fill their slots: finite zeros)
            const int slot = f * P + pl;
            kv[0][slot] = f4{k[0], k[1], k[2], k[3]};
            kv[1][slot] = f4{k[4], k[5], k[6], k[7]};
            kv[2][slot] = f4{v[0], v[1], v[2], v[3]};
            kv[3][slot] = f4{v[4], v[5], v[6], v[7]};
        }
        __syncthreads();
        if (live) {
            float o8[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float m = -INFINITY;
                for (int j = 0; j < F; ++j) {
                    const f4 kj = kv[h][j * P + pl];
                    const float sc = 0.5f * (q[h * 4] * kj[0] + q[h * 4 + 1] * kj[1] + q[h * 4 + 2] * kj[2] + q[h * 4 + 3] * kj[3]);
                    m = fmaxf(m, sc);
                }
                float den = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                for (int j = 0; j < F; ++j) {
                    const f4 kj = kv[h][j * P + pl], vj = kv[2 + h][j * P + pl];
                    const float sc = 0.5f * (q[h * 4] * kj[0] + q[h * 4 + 1] * kj[1] + q[h * 4 + 2] * kj[2] + q[h * 4 + 3] * kj[3]);
                    const float e = expf(sc - m);
                    den += e;
                    a0 = fmaf(e, vj[0], a0); a1 = fmaf(e, vj[1], a1); a2 = fmaf(e, vj[2], a2); a3 = fmaf(e, vj[3], a3);
                }
                o8[h * 4] = a0 / den; o8[h * 4 + 1] = a1 / den; o8[h * 4 + 2] = a2 / den; o8[h * 4 + 3] = a3 / den;
            }
            float x1[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) a = fmaf(o8[i], w[104 + c * 8 + i], a);
                x1[c] = (a + w[136 + c]) + xv[c];
            }
            float hid[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) a = fmaf(x1[c], w[140 + i * 4 + c], a);
                a += w[204 + i];
                hid[i] = 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) a = fmaf(hid[i], w[220 + c * 16 + i], a);
                res[c] = (a + w[284 + c]) + x1[c];
            }
        }
    }
    if (!live) return;
    *(f4*)(out8 + row * 8 + 4) = res;
    if (keep) *(f4*)(keep + row * 4) = res;
    if (sample) {
        f4 sv;
#pragma unroll
        for (int c = 0; c < 4; ++c) sv[c] = load_as_f32(sample, ((b * 4 + c) * F + f) * HW + p, sample_dt);
        *(f4*)(out8 + row * 8) = sv;
    }
}

// adaptive_avg_pool2d of a channels-last map to OH x OW: output (oy, ox) is the mean over input rows [floor(oy H / OH), ceil((oy + 1) H / OH))
// and the like columns -- replication where H < OH.  One thread per output element, channels fastest (dense loads and stores); the
// window is summed in fp32 row by row and divided by its size once (a one-element window is exact).
__global__ __launch_bounds__(256) void adaptive_avgpool_nhwc_kernel(const void* __restrict__ x, int x_dt, void* __restrict__ y, int y_dt,
                                                                    int H, int W, int C, int OH, int OW, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    size_t r = i / C;
    const int ox = (int)(r % OW); r /= OW;
    const int oy = (int)(r % OH);
    const size_t img = r / OH;
    const int y0 = (int)(((long)oy * H) / OH), y1 = (int)((((long)oy + 1) * H + OH - 1) / OH);
    const int x0 = (int)(((long)ox * W) / OW), x1 = (int)((((long)ox + 1) * W + OW - 1) / OW);
    float acc = 0.f;
    for (int iy = y0; iy < y1; ++iy)
        for (int ix = x0; ix < x1; ++ix) acc += load_as_f32(x, ((img * H + iy) * W + ix) * C + c, x_dt);
    store_from_f32(y, i, y_dt, acc / (float)((y1 - y0) * (x1 - x0)));
}

// grid (B), 256 threads.  Row b of out: columns [0, text_dim) the text embedding converted to fp32 (exact for all three dtypes), then
// for id i the embedding diffusers' Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) gives time_ids[b][i]: [cos | sin] of
// id * exp(-ln(10000) k / (dim / 2)).  The sinusoids are computed here, with sincos_kernel's expressions (elementwise.hip), not converted
// from its output: one launch instead of two, and no [B * n_ids][dim] intermediate.
__global__ __launch_bounds__(256) void unet_text_time_kernel(const void* __restrict__ text, int text_dt, int text_dim,
                                                             const float* __restrict__ ids, int n_ids, int dim, float* __restrict__ out,
                                                             long ld_out) {
    const int b = blockIdx.x, half_dim = dim / 2;
    float* row = out + (size_t)b * ld_out;
    for (int c = threadIdx.x; c < text_dim; c += 256) row[c] = load_as_f32(text, (size_t)b * text_dim + c, text_dt);
    for (int j = threadIdx.x; j < n_ids * half_dim; j += 256) {
        const int i = j / half_dim, k = j - i * half_dim;
        const float tv = ids[(size_t)b * n_ids + i];
        const float freq = expf(-9.210340371976184f * (float)k / (float)half_dim);
        const float arg = tv * freq;
        row[text_dim + i * dim + k] = cosf(arg);
        row[text_dim + i * dim + half_dim + k] = sinf(arg);
    }
}

}  // namespace

int op_unet_text_time(const void* text, int text_dt, int text_dim, const float* ids, int n_ids, int dim, float* out, long ld_out, int B,
                      hipStream_t s) {
    CTRL_CHECK(text && ids && out, "unet_text_time: null argument");
    CTRL_CHECK(text_dt >= DT_F32 && text_dt <= DT_BF16, "unet_text_time: text_embeds must be fp32, fp16 or bf16");
    CTRL_CHECK(B >= 1 && B <= 65535 && text_dim >= 1 && n_ids >= 1 && dim >= 2 && dim % 2 == 0 && ld_out >= (long)text_dim + (long)n_ids * dim,
               "unet_text_time: bad sizes (dim even, rows at least text_dim + n_ids * dim wide)");
    PROF_WORK(0, (double)B * ((text_dt == DT_F32 ? 4.0 : 2.0) * text_dim + 4.0 * n_ids + 4.0 * (text_dim + (double)n_ids * dim)));
    prof_detail("B%d text%d ids%d dim%d", B, text_dim, n_ids, dim);
    LAUNCH("unet_text_time", unet_text_time_kernel, dim3((unsigned)B), dim3(256), 0, s, text, text_dt, text_dim, ids, n_ids, dim, out, ld_out);
    return 0;
}

int op_unet_skip_join(const float* skip, long ld_skip, const void* res, int res_dt, int res_5d, int B, int F, int HW, int C2, float* out32,
                      half_t* out16, long ld_out, int col, hipStream_t s, int lo_off) {
    CTRL_CHECK(skip && out32, "unet_skip_join: null argument");
    CTRL_CHECK(lo_off == 0 || (out16 && lo_off % 8 == 0 && lo_off >= col + C2 && (long)lo_off + col + C2 <= 2 * ld_out),
               "unet_skip_join: a split mirror's lo half must lie behind the hi columns, inside the 2 * ld_out wide row");
    CTRL_CHECK(B >= 1 && F >= 1 && HW >= 1 && (long)B * F <= 65535, "unet_skip_join: bad sizes (at most 65535 frames)");
    CTRL_CHECK(C2 >= 32 && C2 % 32 == 0 && col >= 0 && col % 8 == 0 && ld_skip % 8 == 0 && ld_out % 8 == 0 && ld_skip >= C2 && ld_out >= col + C2,
               "unet_skip_join: C2 must be a multiple of 32, the column offset and the row strides multiples of 8, the rows wide enough");
    CTRL_CHECK((((uintptr_t)skip | (uintptr_t)out32 | (uintptr_t)out16) & 15) == 0, "unet_skip_join: pointers must be 16-byte aligned");
    CTRL_CHECK(!res || (res_dt >= DT_F32 && res_dt <= DT_BF16), "unet_skip_join: the residual must be fp32, fp16 or bf16");
    // residual element (b, f, c, p): (b f) c h w -> ((b F + f) C2 + c) HW + p ; b c f h w -> ((b C2 + c) F + f) HW + p
    const long fb = (long)F * C2 * HW, ff = res_5d ? (long)HW : (long)C2 * HW, ch = res_5d ? (long)F * HW : (long)HW;
    const double n = (double)B * F * HW * C2;
    PROF_WORK(0, n * (4.0 + (res ? (res_dt == DT_F32 ? 4.0 : 2.0) : 0.0) + 4.0 + (out16 ? (lo_off ? 4.0 : 2.0) : 0.0)));
    prof_detail("N%d HW%d C%d col%d%s", B * F, HW, C2, col, res ? (res_5d ? " res5d" : " res4d") : "");
    LAUNCH("unet_skip_join", unet_skip_join_kernel, dim3((unsigned)((HW + 63) / 64), (unsigned)(C2 / 32), (unsigned)(B * F)), dim3(256), 0, s,
           skip, ld_skip, res, res_dt, fb, ff, ch, F, HW, C2, out32, out16, ld_out, col, lo_off);
    return 0;
}

int op_unet_conv_out(const half_t* x, const float* w, const float* bias, void* out, int out_dt, int N, int H, int W, int C, int Cout,
                     hipStream_t s, int layout, int frames) {
    CTRL_CHECK(x && w && bias && out, "unet_conv_out: null argument");
    // (a lane walks the 8-channel chunks q, q + 4, ...: with C = 16 two of a pixel's four lanes have no chunk and add zeros)
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 16 && C % 8 == 0 && Cout >= 1 && Cout <= 4, "unet_conv_out: C a multiple of 8 from 16, 1 <= Cout <= 4");
    CTRL_CHECK(layout >= CONV_OUT_NCHW && layout <= CONV_OUT_ROWS && frames >= 1 && (layout != CONV_OUT_NCFHW || N % frames == 0),
               "unet_conv_out: bad output layout (b c f h w needs N to be a multiple of the frames per clip)");
    const long hw = (long)H * W;
    int F = 1;
    long s_b = Cout * hw, s_f = 0, s_c = hw, s_p = 1;                                       // n c h w
    if (layout == CONV_OUT_NCFHW) { F = frames; s_b = (long)Cout * F * hw; s_f = hw; s_c = (long)F * hw; }
    if (layout == CONV_OUT_ROWS) { s_b = hw * Cout; s_c = 1; s_p = Cout; }
    CTRL_CHECK(((uintptr_t)x & 15) == 0, "unet_conv_out: x must be 16-byte aligned");
    CTRL_CHECK(out_dt >= DT_F32 && out_dt <= DT_BF16, "unet_conv_out: bad dtype");
    const size_t npix = (size_t)N * H * W;
    PROF_WORK(2.0 * npix * 9.0 * C * Cout, (double)npix * (2.0 * C + (out_dt == DT_F32 ? 4.0 : 2.0) * Cout));
    prof_detail("N%d %d->%d %dx%d", N, C, Cout, H, W);
    LAUNCH("unet_conv_out", unet_conv_out_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), 0, s, x, w, bias, out, out_dt, N, H, W, C, Cout,
           F, s_b, s_f, s_c, s_p);
    return 0;
}

int op_i2v_frames(const void* x, int dt, float* y, int B, int F, int HW, hipStream_t s) {
    CTRL_CHECK(x && y && B >= 1 && F >= 1 && HW >= 1, "i2v_frames: bad arguments");
    CTRL_CHECK(dt >= DT_F32 && dt <= DT_BF16, "i2v_frames: image_latents must be fp32, fp16 or bf16");
    const size_t n = (size_t)B * F * 4 * HW;
    CTRL_CHECK((n + 255) / 256 <= 0x7fffffffu, "i2v_frames: too many elements");
    PROF_WORK(0, (double)n * ((dt == DT_F32 ? 4.0 : 2.0) + 4.0));
    prof_detail("B%d F%d HW%d", B, F, HW);
    LAUNCH("i2v_frames", i2v_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, dt, y, F, HW, n);
    return 0;
}

int op_i2v_latent_encoder(const float* x, const float* wts, const void* sample, int sample_dt, float* out8, float* keep, int B, int F,
                          int HW, int precomputed, hipStream_t s) {
    CTRL_CHECK(x && out8 && (wts || precomputed), "i2v_latent_encoder: null argument");
    CTRL_CHECK(B >= 1 && F >= 1 && F <= 32 && HW >= 1, "i2v_latent_encoder: 1 .. 32 frames");
    CTRL_CHECK(!sample || (sample_dt >= DT_F32 && sample_dt <= DT_BF16), "i2v_latent_encoder: the sample must be fp32, fp16 or bf16");
    CTRL_CHECK((((uintptr_t)x | (uintptr_t)out8 | (uintptr_t)keep) & 15) == 0, "i2v_latent_encoder: pointers must be 16-byte aligned");
    const int P = 256 / F;
    const size_t npix = (size_t)B * HW, blocks = (npix + P - 1) / P;
    CTRL_CHECK(blocks <= 0x7fffffffu && (double)npix * F * 8.0 < 2147483648.0, "i2v_latent_encoder: too many pixels");
    const double rows = (double)npix * F;
    PROF_WORK(rows * (2.0 * F * 24.0 + 500.0), rows * (16.0 + 32.0 + (keep ? 16.0 : 0.0) + (sample ? 4.0 * (sample_dt == DT_F32 ? 4.0 : 2.0) : 0.0)));
    prof_detail("B%d F%d HW%d%s", B, F, HW, precomputed ? " kept" : "");
    LAUNCH("i2v_latent_encoder", i2v_latent_encoder_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, wts, sample, sample_dt, out8, keep, B,
           F, HW, P, precomputed);
    return 0;
}

int op_adaptive_avgpool_nhwc(const void* x, int x_dt, void* y, int y_dt, int N, int H, int W, int C, int OH, int OW, hipStream_t s) {
    CTRL_CHECK(x && y && N >= 1 && H >= 1 && W >= 1 && C >= 1 && OH >= 1 && OW >= 1, "adaptive_avgpool_nhwc: bad arguments");
    CTRL_CHECK((x_dt == DT_F32 || x_dt == DT_F16) && (y_dt == DT_F32 || y_dt == DT_F16), "adaptive_avgpool_nhwc: fp32 or fp16 maps");
    const size_t n = (size_t)N * OH * OW * C;
    CTRL_CHECK((n + 255) / 256 <= 0x7fffffffu && (double)N * H * W * C < 9.0e18, "adaptive_avgpool_nhwc: too many elements");
    PROF_WORK(0, (double)N * C * ((x_dt == DT_F32 ? 4.0 : 2.0) * H * W + (y_dt == DT_F32 ? 4.0 : 2.0) * OH * OW));
    prof_detail("N%d %dx%d->%dx%d C%d", N, H, W, OH, OW, C);
    LAUNCH("adaptive_avgpool_nhwc", adaptive_avgpool_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, x_dt, y, y_dt, H, W,
           C, OH, OW, n);
    return 0;
}
