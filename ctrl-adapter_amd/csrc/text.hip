// CLIP text encoder kernels (SD-1.5's ViT-L/14 text tower, transformers CLIPTextModel; model/ctrl_helper.py:300-457 runs it):
//   text_embed_ln_kernel   token gather + position add into the fp32 residual stream, fused with layer 0's layer_norm1 (fp16 operand)
//   text_attn_kernel       causal self-attention over L <= 128 tokens, head_dim 64, straight from the Q | K | V GEMM output
//   text_final_kernel      final LayerNorm of every row into the output dtype + the pooled row (index chosen on the device)
//   text_store_kernel      fp32 stream -> output dtype (the hidden_states snapshots)
// The row kernels serve C <= 1024 (SD-1.5's 768); text_embed_ln_wide_kernel and text_final_ext_kernel<8> serve multiples of 64 up to
// 2048 (OpenCLIP bigG's 1280), and text_final_ext_kernel also writes the fp32 pooled row the text projection reads (text_gemm.hip).
// Every kernel computes a row (embedding, norms) or a (prompt, head, 16-query tile) (attention) on its own: a prompt's results do not
// depend on the other prompts of the batch (the plan's batch invariance, plan_text.cpp).
#include "ops.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int kRowThreads = 256;
constexpr int kRowPer = 4;           // C <= kRowThreads * kRowPer (the SD-1.5 kernels)
constexpr int kRowPerWide = 8;       // C <= 2048: the wider towers (OpenCLIP bigG, 1280) in their own instantiations

// sum over the 256 threads of a row workgroup (4 waves), same value in every thread
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();                 // (red is reused by consecutive calls)
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// LayerNorm of the PER values a thread holds (columns threadIdx.x + i * 256 < C), two-pass statistics in fp32
template <int PER>
__device__ __forceinline__ void row_ln(float (&v)[PER], int C, float eps, const float* g, const float* b, float* red) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
    const float mean = block_sum256(s, red) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        const float d = c < C ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum256(q, red) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) v[i] = (v[i] - mean) * rstd * g[c] + b[c];
    }
}

// one workgroup per token row (prompt n, position l): x = tok[clamp(id)] + pos[l] (fp32 stream), y = LayerNorm(x) (fp16)
template <int PER>
__device__ __forceinline__ void text_embed_ln_body(const int64_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                   int V, int L, int C, float* __restrict__ x, const float* __restrict__ g,
                                                   const float* __restrict__ b, float eps, half_t* __restrict__ y, int* __restrict__ bad,
                                                   float* red) {
    const int row = blockIdx.x;
    const int l = row % L;
    int64_t id = ids[row];
    if (id < 0 || id >= V) {         // clamped: no id reads outside the table; the caller learns of it through the flag word
        if (threadIdx.x == 0 && bad) atomicOr(bad, 1);
        id = id < 0 ? 0 : V - 1;
    }
    const float* te = tok + (size_t)id * C;
    const float* pe = pos + (size_t)l * C;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        v[i] = 0.f;
        if (c < C) {
            v[i] = te[c] + pe[c];
            x[(size_t)row * C + c] = v[i];
        }
    }
    row_ln(v, C, eps, g, b, red);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        if (c < C) y[(size_t)row * C + c] = (half_t)v[i];
    }
}

__global__ __launch_bounds__(kRowThreads) void text_embed_ln_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                                    const float* __restrict__ pos, int V, int L, int C, float* __restrict__ x,
                                                                    const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                                    half_t* __restrict__ y, int* __restrict__ bad) {
    __shared__ float red[4];
    text_embed_ln_body<kRowPer>(ids, tok, pos, V, L, C, x, g, b, eps, y, bad, red);
}

// 1024 < C <= 2048
__global__ __launch_bounds__(kRowThreads) void text_embed_ln_wide_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                                         const float* __restrict__ pos, int V, int L, int C, float* __restrict__ x,
                                                                         const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                                         half_t* __restrict__ y, int* __restrict__ bad) {
    __shared__ float red[4];
    text_embed_ln_body<kRowPerWide>(ids, tok, pos, V, L, C, x, g, b, eps, y, bad, red);
}

// pooled position of prompt n (transformers CLIPTextTransformer): eos_id == 2 (the legacy configs SD-1.5 carries) -> the first
// position of the largest id (torch.argmax); otherwise the first position holding eos_id (0 when there is none)
__device__ int pooled_index(const int64_t* ids, int L, int eos, int* red_i) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        int64_t best = INT64_MIN;
        int bi = L;
        for (int l = lane; l < L; l += 64) {
            const int64_t v = ids[l];
            const bool take = eos == 2 ? v > best : (v == eos && bi == L);
            if (take) { best = v; bi = l; }
        }
        if (eos != 2) best = 0;
        // (value desc, index asc) over the wave
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) *red_i = bi >= L ? 0 : bi;
    }
    __syncthreads();
    return *red_i;
}

// one workgroup per row: y[row] = LayerNorm(x[row]) in y_dt; with ids, the prompt's pooled row is also written to pooled[row / L]
// (in y_dt) and, with pooled32, in fp32 to pooled32[row / L] (the text projection's operand)
template <int PER>
__device__ __forceinline__ void text_final_body(const void* __restrict__ x, int x_dt, int C, const float* __restrict__ g,
                                                const float* __restrict__ b, float eps, void* __restrict__ y, int y_dt,
                                                const int64_t* __restrict__ ids, int L, int eos, void* __restrict__ pooled,
                                                float* __restrict__ pooled32, float* red, int* red_i) {
    const int row = blockIdx.x;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        v[i] = c < C ? load_as_f32(x, (size_t)row * C + c, x_dt) : 0.f;
    }
    row_ln(v, C, eps, g, b, red);
    if (y) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = threadIdx.x + i * kRowThreads;
            if (c < C) store_from_f32(y, (size_t)row * C + c, y_dt, v[i]);
        }
    }
    if (ids && (pooled || pooled32)) {
        const int n = row / L;
        if (pooled_index(ids + (size_t)n * L, L, eos, red_i) == row - n * L) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int c = threadIdx.x + i * kRowThreads;
                if (c < C) {
                    if (pooled) store_from_f32(pooled, (size_t)n * C + c, y_dt, v[i]);
                    if (pooled32) pooled32[(size_t)n * C + c] = v[i];
                }
            }
        }
    }
}

// the C <= 1024 kernel is kept as written before text_final_body existed: routed through the body, hipcc commutes three adds of the
// row sum and the ISA would no longer be the SD-1.5 encoder's
__global__ __launch_bounds__(kRowThreads) void text_final_kernel(const void* __restrict__ x, int x_dt, int C, const float* __restrict__ g,
                                                                 const float* __restrict__ b, float eps, void* __restrict__ y, int y_dt,
                                                                 const int64_t* __restrict__ ids, int L, int eos, void* __restrict__ pooled) {
    __shared__ float red[4];
    __shared__ int red_i;
    const int row = blockIdx.x;
    float v[kRowPer];
#pragma unroll
    for (int i = 0; i < kRowPer; ++i) {
        const int c = threadIdx.x + i * kRowThreads;
        v[i] = c < C ? load_as_f32(x, (size_t)row * C + c, x_dt) : 0.f;
    }
    row_ln(v, C, eps, g, b, red);
    if (y) {
#pragma unroll
        for (int i = 0; i < kRowPer; ++i) {
            const int c = threadIdx.x + i * kRowThreads;
            if (c < C) store_from_f32(y, (size_t)row * C + c, y_dt, v[i]);
        }
    }
    if (ids && pooled) {
        const int n = row / L;
        if (pooled_index(ids + (size_t)n * L, L, eos, &red_i) == row - n * L) {
#pragma unroll
            for (int i = 0; i < kRowPer; ++i) {
                const int c = threadIdx.x + i * kRowThreads;
                if (c < C) store_from_f32(pooled, (size_t)n * C + c, y_dt, v[i]);
            }
        }
    }
}

// C <= 256 * PER, with the fp32 pooled row
template <int PER>
__global__ __launch_bounds__(kRowThreads) void text_final_ext_kernel(const void* __restrict__ x, int x_dt, int C, const float* __restrict__ g,
                                                                     const float* __restrict__ b, float eps, void* __restrict__ y, int y_dt,
                                                                     const int64_t* __restrict__ ids, int L, int eos,
                                                                     void* __restrict__ pooled, float* __restrict__ pooled32) {
    __shared__ float red[4];
    __shared__ int red_i;
    text_final_body<PER>(x, x_dt, C, g, b, eps, y, y_dt, ids, L, eos, pooled, pooled32, red, &red_i);
}

__global__ void text_store_kernel(const float* __restrict__ x, void* __restrict__ y, int y_dt, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        store_from_f32(y, i, y_dt, x[i]);
}

// ------------------------------------------------------------------------------------------ causal self-attention
// One wave per (prompt, head, 16-query tile), the (pair, tile) -> workgroup map of the other attention kernels (ops.h attn_work_map:
// whole pairs per XCD, the last partial round dealt over all eight).  The tile's queries, the keys it can see (causal: positions
// < min(L, q0 + 16)) and those values (transposed) sit in LDS; S = Q K^T and O = P V run on v_mfma_f32_16x16x32_f16; the softmax is fp32
// with the mask applied before the row max, P is rounded to fp16 for the second product.  No score reaches HBM.
//   qkv [N*L][ld]: q of head h at column h*64, k at heads*64 + h*64, v at 2*heads*64 + h*64;  out [N*L][ldo], head h at column h*64
constexpr int kQLd = 72;             // halves per Q / K row in LDS (64 + 8: 144-byte rows, 16-byte aligned)

__global__ __launch_bounds__(64) void text_attn_kernel(const half_t* __restrict__ qkv, long ld, half_t* __restrict__ out, long ldo,
                                                       int N, int L, int heads, float scale_log2e, int kpad) {
    extern __shared__ __align__(16) char smem[];
    const int qtiles = (L + 15) >> 4;
    int pair, qt;
    if (!attn_work_map(blockIdx.x, qtiles, N * heads, &pair, &qt)) return;
    const int n = pair / heads, h = pair - n * heads;
    const int q0 = qt * 16;
    const int nk = min(L, q0 + 16);              // keys this tile sees
    const int nkt = (nk + 15) >> 4;              // 16-key tiles of S
    const int nkp = (nk + 31) & ~31;             // key extent of P V (32 per k-step)
    const int vld = kpad + 8;                    // row stride of Vt / P (grid-uniform)
    half_t* Qs = (half_t*)smem;                  // [16][kQLd]
    half_t* Ks = Qs + 16 * kQLd;                 // [kpad][kQLd]
    half_t* Vt = Ks + kpad * kQLd;               // [64][vld]
    half_t* Ps = Vt + 64 * vld;                  // [16][vld]
    const int lane = threadIdx.x;
    const int C = heads * 64;
    const half_t* base = qkv + (size_t)n * L * ld + h * 64;
    const h8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lane; i < 16 * 8; i += 64) {
        const int r = i >> 3, c = (i & 7) * 8;
        *(h8*)(Qs + r * kQLd + c) = q0 + r < L ? *(const h8*)(base + (size_t)(q0 + r) * ld + c) : z8;
    }
    for (int i = lane; i < nkp * 8; i += 64) {   // rows nk..nkp-1 zero: P is 0 there, V must be finite
        const int r = i >> 3, c = (i & 7) * 8;
        h8 kv = z8, vv = z8;
        if (r < nk) {
            kv = *(const h8*)(base + (size_t)r * ld + C + c);
            vv = *(const h8*)(base + (size_t)r * ld + 2 * C + c);
        }
        *(h8*)(Ks + r * kQLd + c) = kv;
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(c + j) * vld + r] = vv[j];
    }
    __syncthreads();

    // S: lane holds A = Q[lr][8 lg + j], B = K^T[8 lg + j][lr] (per 32-wide k-step); C/D: key = 16 jt + lr, query = 4 lg + r
    const int lr = lane & 15, lg = lane >> 4;
    h8 qa[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qa[kk] = *(const h8*)(Qs + lr * kQLd + kk * 32 + lg * 8);
    f4 sv[8];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) {
        if (jt < nkt) {
            f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const h8 kb = *(const h8*)(Ks + (jt * 16 + lr) * kQLd + kk * 32 + lg * 8);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[kk], kb, acc, 0, 0, 0);
            }
            const int key = jt * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + lg * 4 + r;
                const float v = (key <= q && key < L) ? acc[r] * scale_log2e : -INFINITY;     // causal mask before the max
                sv[jt][r] = v;
                mx[r] = fmaxf(mx[r], v);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));     // key 0 is never masked: finite
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) {
        if (jt < nkt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(sv[jt][r] - mx[r]);
                sum[r] += p;
                Ps[(lg * 4 + r) * vld + jt * 16 + lr] = (half_t)p;
            }
        } else if (jt * 16 < nkp) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Ps[(lg * 4 + r) * vld + jt * 16 + lr] = (half_t)0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o, 64);
    __syncthreads();

    // O = P V: A = P[lr][32 ks + 8 lg + j], B = V[32 ks + 8 lg + j][16 dt + lr] = Vt[16 dt + lr][...]; C/D: d = 16 dt + lr, query = 4 lg + r
    f4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < (nkp >> 5); ++ks) {
        const h8 pa = *(const h8*)(Ps + lr * vld + ks * 32 + lg * 8);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const h8 vb = *(const h8*)(Vt + (dt * 16 + lr) * vld + ks * 32 + lg * 8);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, vb, o[dt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + lg * 4 + r;
        if (q < L) {
            const float inv = 1.0f / sum[r];
            half_t* orow = out + ((size_t)n * L + q) * ldo + h * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) orow[dt * 16 + lr] = (half_t)(o[dt][r] * inv);
        }
    }
}

size_t text_attn_lds(int kpad) { return (size_t)2 * (16 * kQLd + kpad * kQLd + 64 * (kpad + 8) + 16 * (kpad + 8)); }

}  // namespace

int op_text_embed(const int64_t* ids, const float* tok, const float* pos, int V, int N, int L, int C, float* x,
                  const float* gamma, const float* beta, float eps, half_t* y, int* bad, hipStream_t s) {
    CTRL_CHECK(ids && tok && pos && x && gamma && beta && y, "text_embed: null argument");
    CTRL_CHECK(N >= 1 && L >= 1 && V >= 1 && C >= 1 && (C <= kRowThreads * kRowPer || (C <= kRowThreads * kRowPerWide && C % 64 == 0)),
               "text_embed: bad shape (C <= 1024, or a multiple of 64 up to 2048)");
    PROF_WORK(0, (double)N * L * C * (4.0 * 2 + 4.0 + 2.0));
    if (C <= kRowThreads * kRowPer)
        LAUNCH("text_embed", text_embed_ln_kernel, dim3(N * L), dim3(kRowThreads), 0, s, ids, tok, pos, V, L, C, x, gamma, beta, eps, y, bad);
    else
        LAUNCH("text_embed", text_embed_ln_wide_kernel, dim3(N * L), dim3(kRowThreads), 0, s, ids, tok, pos, V, L, C, x, gamma, beta, eps, y,
               bad);
    return 0;
}

int op_text_attn(const half_t* qkv, long ld, half_t* out, long ldo, int N, int L, int heads, float scale, hipStream_t s) {
    CTRL_CHECK(qkv && out, "text_attn: null argument");
    CTRL_CHECK(N >= 1 && heads >= 1 && L >= 1 && L <= 128, "text_attn: needs 1 <= L <= 128 tokens");
    CTRL_CHECK(ld % 8 == 0 && ld >= 3L * heads * 64 && ldo >= (long)heads * 64 && ((uintptr_t)qkv & 15) == 0,
               "text_attn: qkv rows must be 16-byte aligned and hold q | k | v (ld >= 3 * heads * 64, ld % 8 == 0)");
    const int qtiles = (L + 15) / 16, pairs = N * heads;
    const int kpad = (L + 31) & ~31;
    const long grid = 8L * ((pairs + 7) / 8) * qtiles;
    CTRL_CHECK(grid < (1L << 31), "text_attn: grid too large");
    // causal: about half of the L x L scores (QK^T and PV, 2 FLOP per MAC)
    PROF_WORK(2.0 * 2.0 * pairs * 64.0 * L * (L + 1) / 2.0, (double)N * L * heads * 64 * 2 * 4);
    LAUNCH("text_attn", text_attn_kernel, dim3((unsigned)grid), dim3(64), text_attn_lds(kpad), s, qkv, ld, out, ldo, N, L, heads,
           scale * 1.4426950408889634f, kpad);
    return 0;
}

int op_text_final(const void* x, int x_dt, int rows, int C, const float* gamma, const float* beta, float eps, void* y, int y_dt,
                  const int64_t* ids, int L, int eos, void* pooled, hipStream_t s) {
    return op_text_final_ext(x, x_dt, rows, C, gamma, beta, eps, y, y_dt, ids, L, eos, pooled, nullptr, s);
}

int op_text_final_ext(const void* x, int x_dt, int rows, int C, const float* gamma, const float* beta, float eps, void* y, int y_dt,
                      const int64_t* ids, int L, int eos, void* pooled, float* pooled32, hipStream_t s) {
    CTRL_CHECK(x && gamma && beta && (y || pooled || pooled32), "text_final: null argument");
    CTRL_CHECK(rows >= 1 && C >= 1 && (C <= kRowThreads * kRowPer || (C <= kRowThreads * kRowPerWide && C % 64 == 0)),
               "text_final: bad shape (C <= 1024, or a multiple of 64 up to 2048)");
    CTRL_CHECK(x_dt >= DT_F32 && x_dt <= DT_BF16 && y_dt >= DT_F32 && y_dt <= DT_BF16, "text_final: bad dtype");
    CTRL_CHECK(!(pooled || pooled32) || (ids && L >= 1 && rows % L == 0), "text_final: the pooled row needs the ids and rows = N * L");
    PROF_WORK(0, (double)rows * C * 8.0);
    const int64_t* pids = (pooled || pooled32) ? ids : nullptr;
    if (C <= kRowThreads * kRowPer && !pooled32)
        LAUNCH("text_final", text_final_kernel, dim3(rows), dim3(kRowThreads), 0, s, x, x_dt, C, gamma, beta, eps, y, y_dt, pids, L, eos, pooled);
    else if (C <= kRowThreads * kRowPer)
        LAUNCH("text_final", text_final_ext_kernel<kRowPer>, dim3(rows), dim3(kRowThreads), 0, s, x, x_dt, C, gamma, beta, eps, y, y_dt, pids,
               L, eos, pooled, pooled32);
    else
        LAUNCH("text_final", text_final_ext_kernel<kRowPerWide>, dim3(rows), dim3(kRowThreads), 0, s, x, x_dt, C, gamma, beta, eps, y, y_dt,
               pids, L, eos, pooled, pooled32);
    return 0;
}

int op_text_store(const float* x, void* y, int y_dt, size_t n, hipStream_t s) {
    CTRL_CHECK(x && y && y_dt >= DT_F32 && y_dt <= DT_BF16, "text_store: bad argument");
    const size_t blocks = std::min<size_t>((n + 255) / 256, 4096);
    PROF_WORK(0, (double)n * (4 + (y_dt == DT_F32 ? 4 : 2)));
    LAUNCH("text_store", text_store_kernel, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(256), 0, s, x, y, y_dt, n);
    return 0;
}
