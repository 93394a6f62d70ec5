// Batch-invariant GEMM for few rows against large weights (the text towers' linears: M = prompts x 77 tokens, N x K up to 5120 x 1280):
//   y[M][N] = act(x[M][K] W^T + b) (+ fp32 residual), x / W fp16, fp32 accumulation, y fp16 or fp32 (the contract of linear() in
//   plan_text.cpp); act 0 none, 2 quick_gelu, 3 exact gelu 0.5 x (1 + erf(x / sqrt 2)).
//
// Two launches:
//   text_gemm_partial_kernel  workgroup = 32 output columns x 512 of K (4 waves, 128 of K each).  A wave loads its 32 x 128 weight slab
//                             into registers ONCE (the B fragments of v_mfma_f32_16x16x32_f16), then walks every row of x in 32-row
//                             passes; the four waves' sums are added in LDS in wave order and the workgroup's partial goes to
//                             ws[split][M][N] (fp32).  The grid is (N / 32) x ceil(K / 512): the weights are read once, spread over all
//                             XCDs; x (M x K fp16, a few hundred KB) is re-read from L2.
//   text_gemm_finish_kernel   y = act(sum over the splits in split order + b) (+ res), one element per thread-vector.
// Batch invariance: the split count, each split's k range, the k order inside a wave (4 MFMA k-steps of 32, fixed) and the reduction
// order (waves 0..3, then splits 0..S-1) are functions of (N, K) alone; every row is computed by the same instruction sequence whatever
// M and whatever its position, so a prompt's bits do not depend on the batch it is in.  No atomics.
#include "ops.h"
#include <algorithm>

namespace {

constexpr int kTgWaves = 4;
constexpr int kTgKW = 128;                   // K per wave
constexpr int kTgKS = kTgWaves * kTgKW;      // K per workgroup (one split)
constexpr int kTgCG = 2;                     // 16-column groups per wave
constexpr int kTgBN = 16 * kTgCG;            // output columns per workgroup
constexpr int kTgRB = 2;                     // 16-row blocks per pass
constexpr int kTgRows = 16 * kTgRB;
constexpr int kTgRedLd = kTgBN + 1;          // LDS row stride of the wave partials (floats)

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == 2) return x_sigmoid_kx(v, 1.702f);                     // quick_gelu, as the igemm epilogue computes it
    if (act == 3) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    return v;
}

__global__ __launch_bounds__(kTgWaves * 64) void text_gemm_partial_kernel(const half_t* __restrict__ x, const half_t* __restrict__ W,
                                                                          int M, int N, int K, float* __restrict__ ws) {
    __shared__ float red[kTgWaves][kTgRows][kTgRedLd];
    const int ntn = (N + kTgBN - 1) / kTgBN;
    const int nt = blockIdx.x % ntn, split = blockIdx.x / ntn;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int n0 = nt * kTgBN;
    const int kw0 = split * kTgKS + wave * kTgKW;
    // k-steps of 32 this wave owns (wave-uniform; K % 32 == 0) and the waves of this split that own any
    const int nsteps = min(max((K - kw0) / 32, 0), kTgKW / 32);
    const int nwaves = min(kTgWaves, (K - split * kTgKS + kTgKW - 1) / kTgKW);
    const h8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // B fragments: lane holds W[n0 + 16 cg + lr][kw0 + 32 ks + 8 lg + j]
    h8 wb[kTgCG][kTgKW / 32];
#pragma unroll
    for (int cg = 0; cg < kTgCG; ++cg) {
        const int n = n0 + cg * 16 + lr;
#pragma unroll
        for (int ks = 0; ks < kTgKW / 32; ++ks)
            wb[cg][ks] = (ks < nsteps && n < N) ? *(const h8*)(W + (size_t)n * K + kw0 + ks * 32 + lg * 8) : z8;
    }

    for (int r0 = 0; r0 < M; r0 += kTgRows) {
        // A fragments: lane holds x[r0 + 16 rb + lr][kw0 + 32 ks + 8 lg + j]
        h8 xa[kTgRB][kTgKW / 32];
#pragma unroll
        for (int rb = 0; rb < kTgRB; ++rb) {
            const int row = r0 + rb * 16 + lr;
#pragma unroll
            for (int ks = 0; ks < kTgKW / 32; ++ks)
                xa[rb][ks] = (ks < nsteps && row < M) ? *(const h8*)(x + (size_t)row * K + kw0 + ks * 32 + lg * 8) : z8;
        }
        f4 acc[kTgRB][kTgCG];
#pragma unroll
        for (int rb = 0; rb < kTgRB; ++rb)
#pragma unroll
            for (int cg = 0; cg < kTgCG; ++cg) {
                acc[rb][cg] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < kTgKW / 32; ++ks)
                    if (ks < nsteps) acc[rb][cg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa[rb][ks], wb[cg][ks], acc[rb][cg], 0, 0, 0);
            }
        // C/D: column 16 cg + lr, row 16 rb + 4 lg + r
#pragma unroll
        for (int rb = 0; rb < kTgRB; ++rb)
#pragma unroll
            for (int cg = 0; cg < kTgCG; ++cg)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave][rb * 16 + lg * 4 + r][cg * 16 + lr] = acc[rb][cg][r];
        __syncthreads();
        for (int e = threadIdx.x; e < kTgRows * kTgBN; e += kTgWaves * 64) {
            const int rr = e / kTgBN, c = e - rr * kTgBN;
            const int row = r0 + rr, n = n0 + c;
            if (row < M && n < N) {
                float s = red[0][rr][c];
                for (int w = 1; w < nwaves; ++w) s += red[w][rr][c];
                ws[((size_t)split * M + row) * N + n] = s;
            }
        }
        __syncthreads();
    }
}

// 4 consecutive columns per thread (N % 4 == 0)
__global__ void text_gemm_finish_kernel(const float* __restrict__ ws, int splits, int M, int N, const float* __restrict__ bias, int act,
                                        const float* __restrict__ res, long ldres, void* __restrict__ y, int y_dt, long ldy) {
    const size_t n4 = (size_t)M * (N / 4);
    const size_t plane = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / (N / 4));
        const int col = (int)(i - (size_t)row * (N / 4)) * 4;
        const size_t o = (size_t)row * N + col;
        f4 v = *(const f4*)(ws + o);
        for (int s = 1; s < splits; ++s) v += *(const f4*)(ws + (size_t)s * plane + o);
        if (bias) v += *(const f4*)(bias + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = apply_act(v[j], act);
        if (res) v += *(const f4*)(res + (size_t)row * ldres + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) store_from_f32(y, (size_t)row * ldy + col + j, y_dt, v[j]);
    }
}

// text_embeds[n][p] = sum_c pooled[n][c] * Wp[p][c], fp32 throughout: one wave per (prompt, output), lanes over c in a fixed order,
// the wave's butterfly sum; a prompt's result depends on its own row alone
__global__ __launch_bounds__(256) void text_proj_kernel(const float* __restrict__ pooled, const float* __restrict__ Wp, int C, int P,
                                                        void* __restrict__ out, int out_dt) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= P) return;
    const float* a = pooled + (size_t)n * C;
    const float* w = Wp + (size_t)p * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(a[c], w[c], s);
    s = wave_sum(s);
    if (lane == 0) store_from_f32(out, (size_t)n * P + p, out_dt, s);
}

}  // namespace

int text_gemm_splits(int N, int K) {
    (void)N;
    return (K + kTgKS - 1) / kTgKS;
}

size_t text_gemm_ws_bytes(int M, int N, int K) { return (size_t)text_gemm_splits(N, K) * M * N * sizeof(float); }

int op_text_gemm_finish(const float* ws, int splits, int M, int N, const float* bias, int act, const float* res, long ldres, void* y,
                        int y_dt, long ldy, hipStream_t s) {
    CTRL_CHECK(ws && y && splits >= 1 && M >= 1 && N >= 4 && N % 4 == 0, "text_gemm_finish: bad argument (N % 4 == 0)");
    CTRL_CHECK(act == 0 || act == 2 || act == 3, "text_gemm_finish: act must be 0, 2 or 3");
    CTRL_CHECK(y_dt >= DT_F32 && y_dt <= DT_BF16 && ldy >= N && (!res || ldres >= N), "text_gemm_finish: bad output");
    const size_t n4 = (size_t)M * (N / 4);
    const size_t blocks = std::max<size_t>(std::min<size_t>((n4 + 255) / 256, 8192), 1);
    PROF_WORK(0, (double)M * N * (4.0 * splits + (res ? 4 : 0) + (y_dt == DT_F32 ? 4 : 2)));
    LAUNCH("text_gemm_fin", text_gemm_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ws, splits, M, N, bias, act, res, ldres, y,
           y_dt, ldy);
    return 0;
}

int op_text_gemm(const half_t* x, const half_t* W, const float* bias, int M, int N, int K, int act, const float* res, void* y, int y_dt,
                 float* ws, size_t ws_bytes, hipStream_t s) {
    CTRL_CHECK(x && W && y && ws, "text_gemm: null argument");
    CTRL_CHECK(M >= 1 && N >= 16 && K >= 32 && N % 16 == 0 && K % 32 == 0, "text_gemm: needs M >= 1, N % 16 == 0, K % 32 == 0");
    CTRL_CHECK((long)M * N <= (1L << 30) && (long)M * K <= (1L << 30) && (long)N * K <= (1L << 30), "text_gemm: problem too large");
    CTRL_CHECK((((uintptr_t)x | (uintptr_t)W) & 15) == 0 && ((uintptr_t)ws & 15) == 0, "text_gemm: x, W and ws must be 16-byte aligned");
    CTRL_CHECK((!bias || ((uintptr_t)bias & 15) == 0) && (!res || ((uintptr_t)res & 15) == 0), "text_gemm: bias / res must be 16-byte aligned");
    // (the finish launch checks these as well: refused here, nothing has been launched yet)
    CTRL_CHECK(act == 0 || act == 2 || act == 3, "text_gemm: act must be 0, 2 or 3");
    CTRL_CHECK(y_dt >= DT_F32 && y_dt <= DT_BF16, "text_gemm: bad output dtype");
    const int splits = text_gemm_splits(N, K);
    CTRL_CHECK(ws_bytes >= text_gemm_ws_bytes(M, N, K), "text_gemm: workspace too small");
    const int ntn = (N + kTgBN - 1) / kTgBN;
    PROF_WORK(2.0 * M * N * K, (double)N * K * 2 + (double)M * K * 2 + (double)splits * M * N * 4);
    LAUNCH("text_gemm", text_gemm_partial_kernel, dim3((unsigned)(ntn * splits)), dim3(kTgWaves * 64), 0, s, x, W, M, N, K, ws);
    return op_text_gemm_finish(ws, splits, M, N, bias, act, res, N, y, y_dt, N, s);
}

int op_text_proj(const float* pooled, const float* Wp, int N, int C, int P, void* out, int out_dt, hipStream_t s) {
    CTRL_CHECK(pooled && Wp && out && N >= 1 && C >= 1 && P >= 1 && out_dt >= DT_F32 && out_dt <= DT_BF16, "text_proj: bad argument");
    CTRL_CHECK(N <= 65535, "text_proj: too many prompts");
    PROF_WORK(2.0 * N * P * C, (double)P * C * 4 + (double)N * C * 4);
    LAUNCH("text_proj", text_proj_kernel, dim3((unsigned)((P + 3) / 4), (unsigned)N), dim3(256), 0, s, pooled, Wp, C, P, out, out_dt);
    return 0;
}
