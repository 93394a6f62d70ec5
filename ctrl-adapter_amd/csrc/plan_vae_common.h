// What the KL-VAE encoder plan (plan_vae.cpp) and decoder plan (plan_vae_decoder.cpp) share: the config checks, a level (ResNets + its
// resampling convolution), the mid block and the two ping-pong stream buffers an image's residual stream walks through.
#pragma once
#include "plan_common.h"
#include <algorithm>

// the checks both halves make on their config (ctrl_vae_encoder_config / ctrl_vae_decoder_config); who = "vae encoder" | "vae decoder"
template <class Cfg>
int validate_vae(const Cfg& c, const std::string& who) {
    CTRL_CHECK(c.num_levels >= 1 && c.num_levels <= 4, who + ": 1 to 4 levels (block_out_channels)");
    for (int i = 0; i < c.num_levels; ++i)
        CTRL_CHECK(c.block_out_channels[i] >= 32 && c.block_out_channels[i] <= 2048 && c.block_out_channels[i] % 32 == 0,
                   who + ": block_out_channels must be multiples of 32 up to 2048");
    CTRL_CHECK(c.layers_per_block >= 1 && c.layers_per_block <= 8, who + ": layers_per_block must be 1 .. 8");
    CTRL_CHECK(c.latent_channels >= 1 && c.latent_channels <= 8, who + ": latent_channels must be 1 .. 8");
    CTRL_CHECK(c.norm_num_groups == 32, who + ": norm_num_groups must be 32");
    CTRL_CHECK(c.norm_eps > 0.f, who + ": norm_eps must be positive");
    return 0;
}

// one resolution level: its ResNets, then (all but the last level) the stride-2 / x2 convolution to the next resolution
struct VaeLevel {
    std::vector<ResnetW> res;
    bool resample = false;
    ConvW conv;
};

// `n` ResNets cin -> cout under `pre`resnets., and `pre``conv_name` when the level resamples; cin leaves as cout
inline int build_vae_level(ParamSink& ps, const std::string& pre, int n, int* cin, int cout, bool resample, const char* conv_name, VaeLevel* lv) {
    lv->res.resize(n);
    for (int j = 0; j < n; ++j) {
        TRY(build_resnet(ps, pre + "resnets." + std::to_string(j), *cin, cout, false, &lv->res[j], true));
        *cin = cout;
    }
    lv->resample = resample;
    if (resample) TRY(ps.conv(pre + conv_name, cout, cout, 3, false, &lv->conv, true));
    return 0;
}

struct VaeMid {
    ResnetW r0, r1;
    Norm attn_gn;
    Lin qkv, attn_out;
};

// half = "encoder." | "decoder."
inline int build_vae_mid(ParamSink& ps, const std::string& half, int Ct, VaeMid* m) {
    TRY(build_resnet(ps, half + "mid_block.resnets.0", Ct, Ct, false, &m->r0, true));
    const std::string ap = half + "mid_block.attentions.0.";
    TRY(ps.norm(ap + "group_norm", Ct, &m->attn_gn));
    TRY(ps.linear_cat({ap + "to_q", ap + "to_k", ap + "to_v"}, {Ct, Ct, Ct}, Ct, true, &m->qkv));
    TRY(ps.linear(ap + "to_out.0", Ct, Ct, true, false, &m->attn_out));
    return build_resnet(ps, half + "mid_block.resnets.1", Ct, Ct, false, &m->r1, true);
}

// The fp32 stream of one image ping-pongs between two buffers of n32 floats; where the next op reads the stream as a convolution
// operand (a shortcut, the resampling conv) the producer also writes its split [hi | lo] fp16 mirror, 2 * n16 halves per buffer.
struct VaeStreams {
    float* s32[2];
    half_t* s16[2];
    int cur = 0;
    VaeStreams(Ctx& cx, size_t n32, size_t n16) {
        s32[0] = cx.f(n32); s32[1] = cx.f(n32);
        s16[0] = n16 ? cx.h(2 * n16) : nullptr; s16[1] = n16 ? cx.h(2 * n16) : nullptr;
    }
    TV first() const { TV v; v.p = s32[0]; v.dt = DT_F32; return v; }      // what the head kernel wrote into s32[0]
    TV next(bool need16, int C) {
        cur ^= 1;
        TV v; v.p = s32[cur]; v.dt = DT_F32; v.m16 = need16 ? s16[cur] : nullptr; v.lo_off = need16 ? C : 0;
        return v;
    }
};

// x <- the level's ResNets, then its resampling convolution (o: stride 2 from tap origin 1, or the x2 up-sampling gather) at h x w.
// A stream gets its fp16 mirror where the next op reads it as a convolution operand: a ResNet with a shortcut -- the next one of this
// level, or the first of the next level (next_first_has_shortcut) behind the resampling -- or the resampling convolution itself.
inline int run_vae_level(Ctx& cx, VaeStreams& st, const VaeLevel& lv, const ConvOpts& o, bool next_first_has_shortcut, TV* x, int h, int w,
                         float eps) {
    const int n = (int)lv.res.size();
    for (int j = 0; j < n; ++j) {
        const bool need16 = j + 1 < n ? lv.res[j + 1].has_shortcut : lv.resample;
        TV y = st.next(need16, lv.res[j].Cout);
        TRY(run_resnet(cx, lv.res[j], *x, y, 1, h, w, 1, nullptr, 0, eps));
        *x = y;
    }
    if (lv.resample) {
        TV y = st.next(next_first_has_shortcut, lv.res.back().Cout);
        TRY(run_conv(cx, lv.conv, x->m16, y, 1, h, w, o));      // the split mirror, as a split operand
        *x = y;
    }
    return 0;
}

// x <- ResNet, attention, ResNet at h x w; need16_after: the op behind the mid block reads the stream as a convolution operand
inline int run_vae_mid(Ctx& cx, VaeStreams& st, const VaeMid& m, TV* x, bool need16_after, int h, int w, float eps) {
    const int Ct = m.attn_gn.C;
    { TV y = st.next(false, Ct); TRY(run_resnet(cx, m.r0, *x, y, 1, h, w, 1, nullptr, 0, eps)); *x = y; }
    { TV y = st.next(false, Ct); TRY(run_vae_mid_attention(cx, m.attn_gn, m.qkv, m.attn_out, Ct, eps, *x, y, h * w)); *x = y; }
    { TV y = st.next(need16_after, Ct); TRY(run_resnet(cx, m.r1, *x, y, 1, h, w, 1, nullptr, 0, eps)); *x = y; }
    return 0;
}
