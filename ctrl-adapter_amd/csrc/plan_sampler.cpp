// ctrl_sampler: the device side of a scheduler -- the fp32 coefficient table (one row per step), the step counter with its ticket word
// and the three timestep scalars the modules read -- and the extern "C" entries of the sampler launches (sampler.hip).
#include "plan_shell.h"

struct Sampler {
    int device = 0;
    int n_steps = 0;
    float* table = nullptr;      // [n_steps][CTRL_SAMPLER_ROW]
    int* counter = nullptr;      // [2]: step, ticket
    float* scalars = nullptr;    // [3]: t_model, t_aux0, t_aux1
    void* block = nullptr;       // the one allocation behind the three
};

extern "C" {

int ctrl_sampler_create(int n_steps, const float* table_fp32_host, ctrl_sampler** out) {
    CTRL_CHECK(out != nullptr, "sampler_create: null argument");
    *out = nullptr;
    CTRL_CHECK(n_steps >= 1 && n_steps <= (1 << 20) && table_fp32_host, "sampler_create: needs a table of 1 .. 2^20 rows");
    Sampler* t = new Sampler();
    t->n_steps = n_steps;
    const size_t tb = al256((size_t)n_steps * CTRL_SAMPLER_ROW * sizeof(float));
    hipError_t e = hipGetDevice(&t->device);
    if (e == hipSuccess) e = hipMalloc(&t->block, tb + 512);
    if (e == hipSuccess) e = hipMemset(t->block, 0, tb + 512);
    if (e == hipSuccess) e = hipMemcpy(t->block, table_fp32_host, (size_t)n_steps * CTRL_SAMPLER_ROW * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (t->block) (void)hipFree(t->block);
        delete t;
        CTRL_FAIL(std::string("sampler_create: ") + hipGetErrorString(e));
    }
    t->table = (float*)t->block;
    t->counter = (int*)((char*)t->block + tb);
    t->scalars = (float*)((char*)t->block + tb + 256);
    *out = (ctrl_sampler*)t;
    return 0;
}

void ctrl_sampler_destroy(ctrl_sampler* h) {
    if (!h) return;
    Sampler* t = (Sampler*)h;
    DeviceGuard dg(t->device);
    (void)hipDeviceSynchronize();        // queued launches and captured graphs may still address the table
    (void)hipFree(t->block);
    delete t;
}

int ctrl_sampler_reset(ctrl_sampler* h, void* stream) {
    CTRL_CHECK(h != nullptr, "sampler_reset: null sampler");
    Sampler* t = (Sampler*)h;
    DeviceGuard dg(t->device);
    return op_sampler_reset(t->counter, S(stream));
}

float* ctrl_sampler_scalars(ctrl_sampler* h) { return h ? ((Sampler*)h)->scalars : nullptr; }

int ctrl_sampler_model_input(ctrl_sampler* h, const ctrl_sampler_desc* d, int step_index, void* stream) {
    CTRL_CHECK(h && d, "sampler_model_input: null argument");
    Sampler* t = (Sampler*)h;
    DeviceGuard dg(t->device);
    return op_sampler(t->table, t->n_steps, t->counter, t->scalars, *d, step_index, false, true, S(stream));
}

int ctrl_sampler_step(ctrl_sampler* h, const ctrl_sampler_desc* d, int step_index, int prepare_next, void* stream) {
    CTRL_CHECK(h && d, "sampler_step: null argument");
    Sampler* t = (Sampler*)h;
    DeviceGuard dg(t->device);
    return op_sampler(t->table, t->n_steps, t->counter, t->scalars, *d, step_index, true, prepare_next != 0, S(stream));
}

int ctrl_op_sampler_reset(int32_t* counter, void* stream) { return op_sampler_reset(counter, S(stream)); }

int ctrl_op_sampler_model_input(const float* table, int n_steps, const int32_t* counter, float* scalars, const ctrl_sampler_desc* d,
                                int step_index, void* stream) {
    CTRL_CHECK(d != nullptr, "sampler_model_input: null descriptor");
    return op_sampler(table, n_steps, (int*)counter, scalars, *d, step_index, false, true, S(stream));
}

int ctrl_op_sampler_step(const float* table, int n_steps, int32_t* counter, float* scalars, const ctrl_sampler_desc* d, int step_index,
                         int prepare_next, void* stream) {
    CTRL_CHECK(d != nullptr, "sampler_step: null descriptor");
    return op_sampler(table, n_steps, counter, scalars, *d, step_index, true, prepare_next != 0, S(stream));
}

int ctrl_op_sampler_launch_shape(const ctrl_sampler_desc* d, int with_step, int with_model_input, int* blocks, int* vec, int* grid_cap) {
    CTRL_CHECK(d && blocks && vec && grid_cap, "sampler_launch_shape: null argument");
    *grid_cap = kSamplerGridCap;
    return sampler_launch_shape(*d, with_step != 0, with_model_input != 0, blocks, vec);
}

}  // extern "C"
