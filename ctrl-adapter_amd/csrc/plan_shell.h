// The shell every plan shares around its own build and forward (included at the end of plan_common.h):
//   * spec_entry: one inventory entry into the C ABI's name / shape / ndim (every ctrl_*_param_spec)
//   * StandalonePlan: packer + workspace of the plans that are one module with one forward (text, vision, VAE encoder, VAE decoder),
//     with plan_create / plan_destroy, the workspace reservation (and its refusal under stream capture) and, for the two plans that
//     size their workspace with a dry pass, the per-image driver
#pragma once
#include "plan_common.h"
#include <cstring>

#define S(stream) ((hipStream_t)(stream))

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t dt_size(int dt) { return dt == DT_F32 ? 4 : 2; }

// entry i of a collected inventory -> name / shape[6] / ndim; `who` is the entry point's name in the range message
inline int spec_entry(const SpecCollector& sc, int i, const char* who, char* name, int name_len, int64_t shape[6], int* ndim) {
    CTRL_CHECK(i >= 0 && i < (int)sc.entries.size(), std::string(who) + ": index out of range");
    std::strncpy(name, sc.entries[i].name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
    *ndim = (int)sc.entries[i].shape.size();
    for (int k = 0; k < 6; ++k) shape[k] = k < *ndim ? sc.entries[i].shape[k] : 1;
    return 0;
}

struct StandalonePlan : PlanBase {
    Packer* pk = nullptr;
    Arena ar;
    ~StandalonePlan() {
        if (pk) { pk->release_all(); delete pk; }
    }
    // the workspace of this forward; `who`: the plan's name in messages, `unit`: what grew ("batch" | "image")
    int reserve(size_t need, bool capturing, const char* who, const char* unit) {
        CTRL_CHECK(!capturing || need <= ar.cap, std::string(who) + ": the first forward of a larger " + unit +
                                                     " allocates its workspace and cannot run under stream capture -- run it eagerly "
                                                     "once, then capture");
        return ar.ensure(need);
    }
};

// ctrl_*_create of a StandalonePlan with a `cfg` member: validate(cfg) before anything is allocated, then the plan on the parameters'
// device, build(packer, plan), post(plan, stream) (packs that follow the build: they join the packer's stream before finish), finish
template <class Plan, class Cfg, class Validate, class Build, class Post>
int plan_create(const char* who, const Cfg* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, void** out, Validate validate,
                Build build, Post post) {
    CTRL_CHECK(cfg && out && (tensors || n_tensors == 0), std::string(who) + ": null argument");
    *out = nullptr;
    TRY(validate(*cfg));
    Plan* t = new Plan();
    t->cfg = *cfg;
    int rc = t->init_base(n_tensors ? tensors[0].data : nullptr);
    DeviceGuard dg(t->device);
    if (!rc) {
        t->pk = new Packer(tensors, n_tensors, S(stream));
        rc = build(*t->pk, *t);
        if (!rc) rc = post(*t, S(stream));
        if (!rc) rc = t->pk->finish();
    }
    if (rc) { delete t; return rc; }
    *out = t;
    return 0;
}

template <class Plan>
void plan_destroy(void* h) {
    if (!h) return;
    Plan* t = (Plan*)h;
    DeviceGuard dg(t->device);
    (void)hipDeviceSynchronize();        // queued launches and captured graphs may still address the workspace
    delete t;
}

// forward of a plan whose images run one after the other through body(cx, n): a dry pass over image 0 sizes the workspace, then the
// real pass over every image from the arena's start.  The two passes must allocate in the same order: body starts with
// `cx.stats_off = 0; begin_forward(cx)`.
template <class Body>
int run_per_image(StandalonePlan& t, int N, hipStream_t s, const char* who, Body body) {
    bool capturing = false;
    TRY(t.enter(s, &capturing));
    t.ar.off = 0; t.ar.peak = 0;
    Ctx dry{&t.ar, s, true};
    TRY(body(dry, 0));
    TRY(t.reserve(workspace_bytes(dry), capturing, who, "image"));
    Ctx cx{&t.ar, s, false};
    cx.capturing = capturing;
    cx.stats_total = dry.stats_total;
    for (int n = 0; n < N; ++n) {
        t.ar.off = 0;
        TRY(body(cx, n));
    }
    return t.leave(s, capturing);
}
