// Samplers (gfx950): the per-step glue of a denoise loop -- scale_model_input, the CFG replicas, the channel concat, the ControlNet's
// rearranged sample, the CFG combine and scheduler.step -- as ONE streaming launch per step.  Every supported scheduler step is linear,
// prev = A_i x + B_i mg, and the model input is c_i x; the host computed the table {c_in, A, B, t_model, t_aux0, t_aux1, 0, 0} in fp64.
// HBM- and launch-bound: 16-byte accesses where the geometry and the pointers allow (SamplerU = 8 elements per thread and trip), a
// scalar path otherwise; one kernel body serves the model-input pass, the step and the fused step + next input, so the fused launch is
// bit-identical to the two it replaces by construction.
#include "ops.h"

namespace {

typedef unsigned short us8 __attribute__((ext_vector_type(8)));

template <int U>
__device__ __forceinline__ void ld_chunk(const void* p, int dt, size_t e, float (&o)[U]) {
    if constexpr (U == 1) {
        o[0] = load_as_f32(p, e, dt);
    } else {
        if (dt == DT_F32) {
            const f4* q = (const f4*)((const float*)p + e);
            const f4 a = q[0], b = q[1];
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
        } else if (dt == DT_F16) {
            const h8 v = *(const h8*)((const half_t*)p + e);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (float)v[j];
        } else {
            const us8 v = *(const us8*)((const u16*)p + e);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = bf16_to_f32(v[j]);
        }
    }
}

// v is already representable in dt (round_dt): the conversions below are exact
template <int U>
__device__ __forceinline__ void st_chunk(void* p, int dt, size_t e, const float (&v)[U]) {
    if constexpr (U == 1) {
        store_from_f32(p, e, dt, v[0]);
    } else {
        if (dt == DT_F32) {
            f4* q = (f4*)((float*)p + e);
            q[0] = f4{v[0], v[1], v[2], v[3]};
            q[1] = f4{v[4], v[5], v[6], v[7]};
        } else if (dt == DT_F16) {
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
            *(h8*)((half_t*)p + e) = o;
        } else {
            us8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = f32_to_bf16(v[j]);
            *(us8*)((u16*)p + e) = o;
        }
    }
}

__device__ __forceinline__ float round_dt(float v, int dt) {
    if (dt == DT_F32) return v;
    if (dt == DT_F16) return (float)(half_t)v;
    return bf16_to_f32(f32_to_bf16(v));
}

struct SamplerArgs {
    SamplerDesc d;
    const float* table;
    int* counter;
    float* scalars;
    size_t n;          // outer * C * inner: elements of the latents
    size_t ncat;       // R * outer * C2 * inner: elements of the concat operand (0: none)
    int n_steps, step_index, with_step, with_input;
};

template <int U>
__global__ __launch_bounds__(256) void sampler_kernel(SamplerArgs a) {
    const SamplerDesc& d = a.d;
    const int i = a.step_index >= 0 ? a.step_index : a.counter[0];
    if (i < 0 || i >= a.n_steps) return;                 // (uniform) a replay beyond the table: nothing is read or written
    const int irow = a.with_step ? i + 1 : i;            // the row the model input is made for
    const bool prep = a.with_input && irow < a.n_steps;
    const float A = a.with_step ? a.table[(size_t)i * CTRL_SAMPLER_ROW + 1] : 0.f;
    const float B = a.with_step ? a.table[(size_t)i * CTRL_SAMPLER_ROW + 2] : 0.f;
    const float cin = prep ? a.table[(size_t)irow * CTRL_SAMPLER_ROW] : 0.f;
    if (prep && blockIdx.x == 0 && threadIdx.x < 3) a.scalars[threadIdx.x] = a.table[(size_t)irow * CTRL_SAMPLER_ROW + 3 + threadIdx.x];

    const size_t CI = (size_t)d.C * d.inner, CCI = (size_t)(d.C + d.C2) * d.inner, C2I = (size_t)d.C2 * d.inner;
    const size_t nch = a.n / U, total = nch + (prep ? a.ncat / U : 0);
    const int hw = d.cn_frames > 0 ? d.inner / d.cn_frames : d.inner;
    for (size_t ch = (size_t)blockIdx.x * 256 + threadIdx.x; ch < total; ch += (size_t)gridDim.x * 256) {
        if (ch < nch) {
            const size_t e = ch * U;
            float v[U];
            ld_chunk<U>(d.x, d.x_dtype, e, v);
            if (a.with_step) {
                float m[U];
                ld_chunk<U>(d.model_out, d.mo_dtype, e, m);
                if (d.R == 2) {
                    float c[U];
                    ld_chunk<U>(d.model_out, d.mo_dtype, a.n + e, c);
                    const float g = d.g ? d.g[(e / (size_t)d.g_inner) % (size_t)d.g_count] : d.g_scalar;
#pragma unroll
                    for (int j = 0; j < U; ++j) m[j] = fmaf(g, c[j] - m[j], m[j]);
                }
#pragma unroll
                for (int j = 0; j < U; ++j) v[j] = round_dt(fmaf(A, v[j], B * m[j]), d.prev_dtype);
                st_chunk<U>(d.prev, d.prev_dtype, e, v);
            }
            if (prep) {
                float w[U];
#pragma unroll
                for (int j = 0; j < U; ++j) w[j] = cin * v[j];
                const size_t o = e / CI, rem = e - o * CI;
                size_t cn_rem = rem;                                     // offset inside one replica's image of the ControlNet's sample
                if (d.cn_frames > 0) {
                    const size_t c = rem / d.inner, j = rem - c * d.inner, f = j / hw, p = j - f * hw;
                    cn_rem = (f * d.C + c) * hw + p;
                }
                for (int r = 0; r < d.R; ++r) {
                    const size_t img = (size_t)r * d.outer + o;
                    float q[U];
#pragma unroll
                    for (int j = 0; j < U; ++j) q[j] = round_dt(w[j], d.unet_dtype);
                    st_chunk<U>(d.unet_in, d.unet_dtype, img * CCI + rem, q);
                    if (d.cn_in) {
#pragma unroll
                        for (int j = 0; j < U; ++j) q[j] = round_dt(w[j], d.cn_dtype);
                        st_chunk<U>(d.cn_in, d.cn_dtype, img * CI + cn_rem, q);
                    }
                }
            }
        } else {
            const size_t e = (ch - nch) * U;                             // the concat operand behind the C channels of every image
            float v[U];
            ld_chunk<U>(d.concat, d.concat_dtype, e, v);
#pragma unroll
            for (int j = 0; j < U; ++j) v[j] = round_dt(v[j], d.unet_dtype);
            const size_t img = e / C2I, rem = e - img * C2I;
            st_chunk<U>(d.unet_in, d.unet_dtype, img * CCI + CI + rem, v);
        }
    }
    // the device counter: every THREAD of a workgroup read it above (the early return branches on the value, so the load has
    // completed), and the barrier holds thread 0 back until all four waves of its workgroup are past that read and done with their
    // chunks -- only then does the workgroup draw its ticket (as the GroupNorm statistics' ticket does).  The workgroup that draws the
    // last ticket may therefore advance the counter: no wave of this launch is left to read the old value.  The ticket word is left
    // zero for the next launch, as split-K's ticket words are.  (The early return is uniform over the launch: the barrier is legal.)
    if (a.with_step && a.step_index < 0) {
        __syncthreads();
    }
    if (a.with_step && a.step_index < 0 && threadIdx.x == 0) {
        __threadfence();
        const unsigned t = atomicAdd((unsigned*)&a.counter[1], 1u);
        if (t == gridDim.x - 1) {
            a.counter[1] = 0;
            a.counter[0] = i + 1;
        }
    }
}

__global__ void sampler_reset_kernel(int* counter) {
    if (threadIdx.x < 2) counter[threadIdx.x] = 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int sampler_launch_shape(const SamplerDesc& d, bool with_step, bool with_input, int* blocks, int* vec) {
    CTRL_CHECK(with_step || with_input, "sampler: nothing to do");
    CTRL_CHECK(d.outer >= 1 && d.C >= 1 && d.inner >= 1 && d.C2 >= 0, "sampler: outer, C, inner must be positive");
    CTRL_CHECK(d.R == 1 || d.R == 2, "sampler: R must be 1 or 2");
    CTRL_CHECK(d.x != nullptr && d.x_dtype >= DT_F32 && d.x_dtype <= DT_BF16, "sampler: the latents need a pointer and a dtype of fp32 / fp16 / bf16");
    const size_t n = (size_t)d.outer * d.C * d.inner;
    CTRL_CHECK(n * d.R * (size_t)(1 + d.C2) < ((size_t)1 << 40), "sampler: tensor too large");
    bool v8 = d.inner % 8 == 0 && aligned16(d.x);
    if (with_step) {
        CTRL_CHECK(d.model_out && d.prev, "sampler step: model_out and prev are required");
        CTRL_CHECK(d.mo_dtype >= DT_F32 && d.mo_dtype <= DT_BF16 && d.prev_dtype >= DT_F32 && d.prev_dtype <= DT_BF16, "sampler step: bad dtype");
        CTRL_CHECK(d.prev != d.x || d.prev_dtype == d.x_dtype, "sampler step: in place needs prev_dtype == x_dtype");
        CTRL_CHECK(!with_input || d.prev_dtype == d.x_dtype, "sampler step: the fused next input works from prev in the latents' dtype");
        if (d.R == 2 && d.g) {
            CTRL_CHECK(d.g_count >= 1 && d.g_inner >= 1, "sampler step: g_count and g_inner must be positive");
            v8 = v8 && d.g_inner % 8 == 0;
        }
        v8 = v8 && aligned16(d.model_out) && aligned16(d.prev);
    }
    if (with_input) {
        CTRL_CHECK(d.unet_in != nullptr && d.unet_dtype >= DT_F32 && d.unet_dtype <= DT_BF16, "sampler model input: unet_in and its dtype are required");
        CTRL_CHECK((d.C2 > 0) == (d.concat != nullptr), "sampler model input: concat and C2 go together");
        CTRL_CHECK(!d.concat || (d.concat_dtype >= DT_F32 && d.concat_dtype <= DT_BF16), "sampler model input: bad concat dtype");
        CTRL_CHECK(!d.cn_in || (d.cn_dtype >= DT_F32 && d.cn_dtype <= DT_BF16), "sampler model input: bad ControlNet sample dtype");
        CTRL_CHECK(d.cn_frames >= 0 && (d.cn_frames == 0 || d.inner % d.cn_frames == 0), "sampler model input: cn_frames must divide inner");
        CTRL_CHECK(d.unet_in != d.x && d.unet_in != d.prev && d.cn_in != d.x && (!d.cn_in || d.cn_in != d.prev),
                   "sampler model input: the outputs must not alias the latents");
        v8 = v8 && aligned16(d.unet_in) && aligned16(d.concat) && aligned16(d.cn_in);
        if (d.cn_in && d.cn_frames > 0) v8 = v8 && (d.inner / d.cn_frames) % 8 == 0;
    }
    const size_t ncat = with_input && d.concat ? (size_t)d.R * d.outer * d.C2 * d.inner : 0;
    const int U = v8 ? 8 : 1;
    size_t b = ((n + ncat) / U + 255) / 256;
    if (b > (size_t)kSamplerGridCap) b = kSamplerGridCap;
    if (b < 1) b = 1;
    *blocks = (int)b;
    *vec = U;
    return 0;
}

int op_sampler(const float* table, int n_steps, int* counter, float* scalars, const SamplerDesc& d, int step_index, bool with_step,
               bool with_input, hipStream_t s) {
    CTRL_CHECK(table && n_steps >= 1, "sampler: no coefficient table");
    CTRL_CHECK(step_index >= -1 && step_index < n_steps, "sampler: step_index beyond the table (-1 = the device counter)");
    CTRL_CHECK(step_index >= 0 || counter, "sampler: step_index -1 needs the device counter");
    CTRL_CHECK(!with_input || scalars, "sampler: the model-input pass needs the scalar buffer");
    int blocks = 0, U = 0;
    TRY(sampler_launch_shape(d, with_step, with_input, &blocks, &U));
    SamplerArgs a;
    a.d = d;
    a.table = table; a.counter = counter; a.scalars = scalars;
    a.n = (size_t)d.outer * d.C * d.inner;
    a.ncat = with_input && d.concat ? (size_t)d.R * d.outer * d.C2 * d.inner : 0;
    a.n_steps = n_steps; a.step_index = step_index; a.with_step = with_step; a.with_input = with_input;
    const double es[3] = {4.0, 2.0, 2.0};
    PROF_WORK(0, (double)a.n * ((with_step ? es[d.x_dtype] + d.R * es[d.mo_dtype] + es[d.prev_dtype] : es[d.x_dtype]) +
                                (with_input ? d.R * (es[d.unet_dtype] + (d.cn_in ? es[d.cn_dtype] : 0.0)) : 0.0)) +
                         (double)a.ncat * (with_input && d.concat ? es[d.concat_dtype] + es[d.unet_dtype] : 0.0));
    if (U == 8) LAUNCH("sampler", sampler_kernel<8>, dim3(blocks), dim3(256), 0, s, a);
    else LAUNCH("sampler", sampler_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
    return 0;
}

int op_sampler_reset(int* counter, hipStream_t s) {
    CTRL_CHECK(counter != nullptr, "sampler_reset: null counter");
    LAUNCH("sampler", sampler_reset_kernel, dim3(1), dim3(64), 0, s, counter);
    return 0;
}
