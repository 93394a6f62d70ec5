// Kernels of the backbone UNets (SVD: plan_unet_st.cpp, SDXL: plan_unet2d.cpp; gfx950) that no other plan has:
//   unet_skip_join_kernel   one skip tensor of the up path: fp32 NHWC skip (+ the adapter's residual, read in the caller's NCHW / NCFHW
//                           layout) -> columns [col, col + C2) of the up ResNet's concatenated operand, fp32 master + fp16 mirror
//   unet_conv_out_kernel    conv_out 3x3, C0 -> <= 4 channels, on the normalised + activated fp16 map -> NCHW in the sample's dtype
//   unet_text_time_kernel   SDXL's text_time addition embedding: the operand rows of add_embedding.linear_1, [text_embeds | sinusoids of
//                           the time ids], in one launch (a few KB: latency only)
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
                                                            int H, int W, int C, int Cout) {
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
    const size_t hw = (size_t)H * W, p = (size_t)oy * W + ox;
    for (int o = 0; o < Cout; ++o) store_from_f32(out, ((size_t)n * Cout + o) * hw + p, out_dt, acc[o] + bias[o]);
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
                     hipStream_t s) {
    CTRL_CHECK(x && w && bias && out, "unet_conv_out: null argument");
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && Cout >= 1 && Cout <= 4, "unet_conv_out: C a multiple of 32, 1 <= Cout <= 4");
    CTRL_CHECK(((uintptr_t)x & 15) == 0, "unet_conv_out: x must be 16-byte aligned");
    CTRL_CHECK(out_dt >= DT_F32 && out_dt <= DT_BF16, "unet_conv_out: bad dtype");
    const size_t npix = (size_t)N * H * W;
    PROF_WORK(2.0 * npix * 9.0 * C * Cout, (double)npix * (2.0 * C + (out_dt == DT_F32 ? 4.0 : 2.0) * Cout));
    prof_detail("N%d %d->%d %dx%d", N, C, Cout, H, W);
    LAUNCH("unet_conv_out", unet_conv_out_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), 0, s, x, w, bias, out, out_dt, N, H, W, C, Cout);
    return 0;
}
