// extern "C" op-level entry points of libctrlhip (thin: validate, cast, forward to the op layer).
#include "plan_shell.h"

#define H(p) ((half_t*)(p))
#define CH(p) ((const half_t*)(p))

extern "C" {
int ctrl_op_igemm(const ctrl_igemm_desc* d, void* stream) {
    CTRL_CHECK(d != nullptr, "igemm: null descriptor");
    return op_igemm(*d, S(stream));
}
int ctrl_op_igemm_pinned(const ctrl_igemm_desc* d, void* stream) {
    CTRL_CHECK(d != nullptr, "igemm_pinned: null descriptor");
    return op_igemm_pinned(*d, S(stream));
}
int ctrl_op_igemm_group(const ctrl_igemm_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr, "igemm_group: null descriptor array");
    return op_igemm_group(d, n, S(stream));
}
int ctrl_igemm_splitk_factor(const ctrl_igemm_desc* d) { return d ? igemm_splitk_factor(*d) : 0; }
int64_t ctrl_igemm_splitk_ws_bytes(const ctrl_igemm_desc* d, int splits) { return d ? (int64_t)igemm_splitk_ws_bytes(*d, splits) : 0; }
int64_t ctrl_igemm_splitk_ticket_words(const ctrl_igemm_desc* d, int splits) { return d ? (int64_t)igemm_splitk_ticket_words(*d, splits) : 0; }
int ctrl_igemm_select(const ctrl_igemm_desc* d, int group_n, int pinned, char* buf, int cap) {
    CTRL_CHECK(d != nullptr, "igemm_select: null descriptor");
    return igemm_select_text(*d, group_n, pinned != 0, buf, cap);
}
int ctrl_op_ffn(const ctrl_ffn_desc* d, void* stream) {
    CTRL_CHECK(d != nullptr, "ffn: null descriptor");
    return op_ffn_fused_group(d, 1, S(stream));
}
int ctrl_op_ffn_group(const ctrl_ffn_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr, "ffn_group: null descriptor array");
    return op_ffn_fused_group(d, n, S(stream));
}
int ctrl_op_ffn_pack_w2(const void* w2_packed, void* out, int N, int K, void* stream) {
    CTRL_CHECK(w2_packed && out, "ffn_pack_w2: null argument");
    return op_ffn_pack_w2((const half_t*)w2_packed, (half_t*)out, N, K, S(stream));
}
int ctrl_igemm_set_order(const char* spec) { return igemm_set_order(spec); }
int ctrl_igemm_set_wide(int mode) {
    CTRL_CHECK(mode >= -1 && mode <= 2, "igemm_set_wide: mode must be -1 (default), 0 (never), 1 (auto) or 2 (every eligible problem)");
    return igemm_set_wide(mode);
}
int ctrl_igemm_tile_of(int bid, int ntm, int ntn, int mode, int group, int* tile_m, int* tile_n) {
    CTRL_CHECK(tile_m && tile_n && ntm > 0 && ntn > 0 && bid >= 0 && bid < ntm * ntn, "igemm_tile_of: bad arguments");
    igemm_tile_of(bid, ntm, ntn, mode, group, tile_m, tile_n);
    return 0;
}
int ctrl_op_flash_attn(const ctrl_attn_desc* d, void* stream) {
    CTRL_CHECK(d != nullptr, "flash_attn: null descriptor");
    return op_flash_attn(*d, S(stream));
}
int ctrl_op_flash_attn_group(const ctrl_attn_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr, "flash_attn_group: null descriptor array");
    return op_flash_attn_group(d, n, S(stream));
}
int ctrl_attn_set_variant(int v) {
    CTRL_CHECK(v >= -1 && v <= 14, "attn_set_variant: variant out of range (-1 = default, 0 = round-2 kernel, 1..14 = attention_d64.hip)");
    return attn_set_variant(v);
}
int ctrl_attn_work_map(int gbid, int qtiles, int pairs, int* pair, int* qtile) {
    if (!pair || !qtile || gbid < 0 || qtiles < 1 || pairs < 1) return 0;
    return attn_work_map(gbid, qtiles, pairs, pair, qtile) ? 1 : 0;
}
int ctrl_op_temporal_attn(const ctrl_tattn_desc* d, void* stream) {
    CTRL_CHECK(d != nullptr, "temporal_attn: null descriptor");
    return op_temporal_attn(*d, S(stream));
}
size_t ctrl_op_gn_stats_floats(int imgs, int rows_per_img, int C, int G) { return op_gn_stats_floats(imgs, rows_per_img, C, G); }
int ctrl_op_gn_stats(const void* x, int x_dtype, float* stats, int imgs, int rows_per_img, int C, int G, void* stream) {
    return op_gn_stats(x, x_dtype, stats, imgs, rows_per_img, C, G, S(stream));
}
int ctrl_op_gn_apply(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y,
                     int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream) {
    return op_gn_apply(x, x_dtype, stats, gamma, beta, H(y), imgs, rows_per_img, C, G, eps, silu, S(stream));
}
int ctrl_op_gn_fused_applies(int x_dtype, int rows_per_img, int C, int G) { return op_gn_fused_fits(x_dtype, rows_per_img, C, G) ? 1 : 0; }
int ctrl_op_gn_fused(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int64_t ldy, int lo_off,
                     int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream) {
    return op_gn_fused(x, x_dtype, gamma, beta, H(y), imgs, rows_per_img, C, G, eps, silu, S(stream), (long)ldy, lo_off);
}
int ctrl_op_gn_apply_split(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y,
                           int64_t ldy, int lo_off, int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream) {
    return op_gn_apply(x, x_dtype, stats, gamma, beta, H(y), imgs, rows_per_img, C, G, eps, silu, S(stream), (long)ldy, lo_off);
}
int ctrl_op_layernorm(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                      int M, int C, float eps, void* stream) {
    return op_layernorm(x, x_dtype, ldx, gamma, beta, H(y), ldy, M, C, eps, S(stream));
}
// the test ABI of the norm and streaming kernels (tests/test_gpu_norm_forms.py, tests/test_gpu_stream_forms.py): every argument of the
// op layer, the grouped launches, and the launch-shape query -- no logic of their own
static GnStatsArgs gn_stats_args(const ctrl_gn_desc& d) {
    return GnStatsArgs{d.x, d.x_dtype, d.stats, d.imgs, d.rows_per_img, d.C, d.G, (long)d.ldx};
}
static GnApplyArgs gn_apply_args(const ctrl_gn_desc& d) {
    return GnApplyArgs{d.x, d.x_dtype, d.stats, d.gamma, d.beta, H(d.y), d.imgs, d.rows_per_img, d.C, d.G, d.eps, d.silu, (long)d.ldy, d.lo_off,
                       (long)d.stat_rows, (long)d.y_img_rows, (long)d.y_row0, (long)d.ldx};
}
int ctrl_op_gn_stats_group(const ctrl_gn_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr && n >= 1 && n <= kMaxGroup, "gn_stats_group: 1..4 descriptors");
    GnStatsArgs a[kMaxGroup];
    for (int i = 0; i < n; ++i) a[i] = gn_stats_args(d[i]);
    return op_gn_stats_group(a, n, S(stream));
}
int ctrl_op_gn_apply_group(const ctrl_gn_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr && n >= 1 && n <= kMaxGroup, "gn_apply_group: 1..4 descriptors");
    GnApplyArgs a[kMaxGroup];
    for (int i = 0; i < n; ++i) a[i] = gn_apply_args(d[i]);
    return op_gn_apply_group(a, n, S(stream));
}
int ctrl_op_gn_fused_group(const ctrl_gn_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr && n >= 1 && n <= kMaxGroup, "gn_fused_group: 1..4 descriptors");
    GnApplyArgs a[kMaxGroup];
    for (int i = 0; i < n; ++i) a[i] = gn_apply_args(d[i]);
    return op_gn_fused_group(a, n, S(stream));
}
int ctrl_gn_launch_shape(int imgs, int rows_per_img, int C, int pass, int* rows_per_block, int* chunks) {
    CTRL_CHECK(gn_launch_shape(imgs, rows_per_img, C, pass, rows_per_block, chunks), "gn_launch_shape: bad arguments");
    return 0;
}
static LnArgs ln_args(const ctrl_ln_desc& d) {
    return LnArgs{d.x, d.x_dtype, (long)d.ldx, d.addv, (long)d.ldv, d.rows_per_img, d.vmod, d.xsum, d.gamma, d.beta, H(d.y), (long)d.ldy, d.M, d.C,
                  d.eps};
}
int ctrl_op_layernorm_group(const ctrl_ln_desc* d, int n, void* stream) {
    CTRL_CHECK(d != nullptr && n >= 1 && n <= kMaxGroup, "layernorm_group: 1..4 descriptors");
    LnArgs a[kMaxGroup];
    for (int i = 0; i < n; ++i) a[i] = ln_args(d[i]);
    return op_layernorm_group(a, n, S(stream));
}
int ctrl_op_layernorm_add(const void* x, int x_dtype, int64_t ldx, const float* addv, int64_t ldv, int rows_per_img, int vmod, void* xsum,
                          const float* gamma, const float* beta, void* y, int64_t ldy, int M, int C, float eps, void* stream) {
    return op_layernorm_add(x, x_dtype, ldx, addv, ldv, rows_per_img, vmod, xsum, gamma, beta, H(y), ldy, M, C, eps, S(stream));
}
int ctrl_op_add_rowvec_clip(const void* x, int x_dtype, const float* v, int64_t ldv, void* y, int y_dtype, int B, int F, int L, int C,
                            void* stream) {
    return op_add_rowvec_clip(x, x_dtype, v, ldv, y, y_dtype, B, F, L, C, S(stream));
}
int ctrl_op_upsample2x_nhwc(const void* x, void* y, int N, int H, int W, int C, void* stream) {
    CTRL_CHECK(x && y && N >= 1 && H >= 1 && W >= 1, "upsample2x_nhwc: bad arguments");
    return op_upsample2x_nhwc(CH(x), H(y), N, H, W, C, S(stream));
}
int ctrl_op_fill_zero_group(void* const* p, const size_t* bytes, int n, void* stream) {
    return op_fill_zero_group(p, bytes, n, S(stream));
}
int ctrl_op_linear_small_group(const ctrl_small_lin* p, int count, void* stream) {
    CTRL_CHECK(p != nullptr && count >= 1 && count <= 4096, "linear_small_group: 1..4096 problems");
    std::vector<SmallLin> q((size_t)count);
    for (int i = 0; i < count; ++i)
        q[i] = SmallLin{p[i].x, (long)p[i].ldx, CH(p[i].w), p[i].b, p[i].out, (long)p[i].ldo, p[i].M, p[i].N, p[i].K, p[i].in_silu, p[i].out_silu};
    return op_linear_small_group(q.data(), count, S(stream));
}
int ctrl_op_frameidx_sincos(float* out, int N, int F, int dim, void* stream) {
    CTRL_CHECK(out && N >= 1 && F >= 1 && dim >= 2 && dim % 2 == 0, "frameidx_sincos: bad arguments");
    return op_frameidx_sincos(out, N, F, dim, S(stream));
}
int ctrl_op_nchw_to_nhwc(const void* x, int dtype, void* y, int N, int C, int HW, void* stream) {
    return op_nchw_to_nhwc(x, dtype, H(y), N, C, HW, S(stream));
}
int ctrl_op_nhwc_to_nchw(const void* x, void* y, int dtype, int N, int C, int HW, float scale, void* stream) {
    return op_nhwc_to_nchw(CH(x), y, dtype, N, C, HW, scale, S(stream));
}
int ctrl_avgpool_nchw(const void* x, void* y, int dtype, int NC, int Hin, int Win, int Hout, int Wout, void* stream) {
    return op_avgpool_nchw(x, y, dtype, NC, Hin, Win, Hout, Wout, S(stream));
}
int ctrl_op_timestep_sincos(const float* t, int t_count, float* out, int N, int dim, void* stream) {
    return op_timestep_sincos(t, t_count, out, N, dim, S(stream));
}
int ctrl_op_linear_small(const float* x, int64_t ldx, const void* w, const float* b, float* out, int64_t ldo,
                         int M, int N, int K, int in_silu, int out_silu, void* stream) {
    return op_linear_small(x, ldx, CH(w), b, out, ldo, M, N, K, in_silu, out_silu, S(stream));
}
int ctrl_op_blend(const void* xs, int xs_dtype, const void* xt, int xt_dtype, const float* mix, void* y, int y_dtype, size_t n, void* stream) {
    return op_blend(xs, xs_dtype, xt, xt_dtype, mix, y, y_dtype, n, S(stream));
}
int ctrl_op_add_rowvec(const void* x, int x_dtype, const float* v, int64_t ldv, void* y, int y_dtype, size_t M, int C, int rows_per_img, int vmod, void* stream) {
    return op_add_rowvec(x, x_dtype, v, ldv, y, y_dtype, M, C, rows_per_img, vmod, S(stream));
}
int ctrl_op_conv3x3_direct(const void* in, int in_dtype, int in_nchw, const float* w, const float* bias, void* out,
                           int N, int Cin, int Cout, int Hin, int Win, int stride, int silu, void* stream) {
    return op_conv3x3_direct(in, in_dtype, in_nchw, w, bias, H(out), N, Cin, Cout, Hin, Win, stride, silu, S(stream));
}
int ctrl_op_conv3x3_direct_f32(const void* in, int in_dtype, const float* w, const float* bias, void* out, int N, int Cin, int Cout,
                               int H, int W, void* stream) {
    CTRL_CHECK(in && w && out && N >= 1 && H >= 1 && W >= 1, "conv3x3_direct_f32: bad arguments");
    return op_conv3x3_direct_f32(in, in_dtype, w, bias, (float*)out, N, Cin, Cout, H, W, S(stream));
}
int ctrl_op_conv3x3_rows_f32(const void* in, const float* w, const float* bias, void* out, int N, int Cin, int Cout, int H, int W,
                             void* stream) {
    CTRL_CHECK(in && w && out && N >= 1 && H >= 1 && W >= 1, "conv3x3_rows_f32: bad arguments");
    return op_conv3x3_rows_f32((const float*)in, w, bias, (float*)out, N, Cin, Cout, H, W, S(stream));
}
int ctrl_op_conv3x3_small_mfma(const void* x, const void* w, const float* bias, void* out, int N, int Cin, int Cout, int Hin, int Win,
                               int stride, int silu, void* stream) {
    return op_conv3x3_small_mfma((const half_t*)x, (const half_t*)w, bias, H(out), N, Cin, Cout, Hin, Win, stride, silu, S(stream));
}
int ctrl_op_pack_conv_w_phase(const void* w, int dtype, void* out, int Cout, int Cin, void* stream) {
    CTRL_CHECK(w && out && Cout > 0 && Cin > 0, "pack_conv_w_phase: bad arguments");
    return op_pack_conv_w_phase(w, dtype, H(out), Cout, Cin, S(stream));
}
int ctrl_op_pack_conv_w(const void* w, int dtype, void* out, int Cout, int Cin, int taps, void* stream) {
    return op_pack_conv_w(w, dtype, H(out), Cout, Cin, taps, S(stream));
}
int ctrl_op_pack_conv_w_dup(const void* w, int dtype, void* out, int Cout, int Cin, int taps, void* stream) {
    return op_pack_conv_w_dup(w, dtype, H(out), Cout, Cin, taps, S(stream));
}
int ctrl_op_pack_conv_w_direct(const void* w, int dtype, float* out, int Cout, int Cin, void* stream) {
    return op_pack_conv_w_direct(w, dtype, out, Cout, Cin, S(stream));
}
int ctrl_op_pack_linear_w(const void* w, int dtype, void* out, int N, int K, int geglu, void* stream) {
    return op_pack_linear_w(w, dtype, H(out), N, K, geglu, S(stream));
}
int ctrl_op_pack_vec(const void* v, int dtype, float* out, int N, int geglu, void* stream) {
    return op_pack_vec(v, dtype, out, N, geglu, S(stream));
}
// test ABI of the helper kernels (tests/helper_forms.py): the packers with the caller's fp16 range flag, the transpose with an image map,
// and the three per-pixel kernels only a plan reached
int ctrl_op_pack_conv_w_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int taps, int32_t* ovf, void* stream) {
    return op_pack_conv_w(w, dtype, H(out), Cout, Cin, taps, S(stream), ovf);
}
int ctrl_op_pack_conv_w_dup_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int taps, int32_t* ovf, void* stream) {
    return op_pack_conv_w_dup(w, dtype, H(out), Cout, Cin, taps, S(stream), ovf);
}
int ctrl_op_pack_conv_w_phase_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int32_t* ovf, void* stream) {
    return op_pack_conv_w_phase(w, dtype, H(out), Cout, Cin, S(stream), ovf);
}
int ctrl_op_pack_linear_w_ovf(const void* w, int dtype, void* out, int N, int K, int geglu, int32_t* ovf, void* stream) {
    return op_pack_linear_w(w, dtype, H(out), N, K, geglu, S(stream), ovf);
}
int ctrl_op_nhwc_to_nchw_map(const void* x, void* y, int dtype, int N, int C, int HW, float scale, const int32_t* img_map, void* stream) {
    return op_nhwc_to_nchw(CH(x), y, dtype, N, C, HW, scale, S(stream), img_map);
}
int ctrl_op_unet_conv_out(const void* x, const float* w, const float* bias, void* out, int out_dtype, int N, int H, int W, int C, int Cout,
                          int layout, int frames, void* stream) {
    return op_unet_conv_out(CH(x), w, bias, out, out_dtype, N, H, W, C, Cout, S(stream), layout, frames);
}
int ctrl_op_i2v_frames(const void* x, int dtype, float* y, int B, int F, int HW, void* stream) {
    return op_i2v_frames(x, dtype, y, B, F, HW, S(stream));
}
int ctrl_op_vae_conv_in(const void* px, int dtype, const float* w, const float* b, float* out, int H, int W, int Cout, void* stream) {
    return op_vae_conv_in(px, dtype, w, b, out, H, W, Cout, S(stream));
}
int ctrl_router_weights(const float* wg, const int* mask_host, float* weights_out, int R, int E, int equal_weights, void* stream) {
    return op_router_softmax(wg, mask_host, weights_out, R, E, equal_weights, S(stream));
}
int ctrl_router_merge(const void* const* experts_host, const float* weights_row, const int* widx_host, int K,
                      void* out, int dtype, size_t n, void* stream) {
    return op_weighted_merge(experts_host, weights_row, widx_host, K, out, dtype, n, S(stream));
}
static int merge_slots(const ctrl_merge_slot* p, int n, MergeSlot* q) {
    CTRL_CHECK(p && n >= 1 && n <= CTRL_MERGE_SLOTS, "merge_gather: 1..13 slots");
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 8; ++k) q[i].in[k] = p[i].in[k];
        q[i].out = p[i].out; q[i].elems = (long)p[i].elems; q[i].row = p[i].row;
    }
    return 0;
}
int ctrl_op_merge_gather_group(const ctrl_merge_slot* slots, int n_slots, const float* w, int R, int E, const int* widx_host, int K,
                               const int32_t* map, int n_in, int n_out, int in_dtype, int out_dtype, void* stream) {
    MergeSlot q[CTRL_MERGE_SLOTS];
    TRY(merge_slots(slots, n_slots, q));
    return op_merge_gather_group(q, n_slots, w, R, E, widx_host, K, map, n_in, n_out, in_dtype, out_dtype, S(stream));
}
int ctrl_op_merge_gather_launch_shape(const ctrl_merge_slot* slots, int n_slots, const float* w, int R, int E, const int* widx_host, int K,
                                      const int32_t* map, int n_in, int n_out, int in_dtype, int out_dtype, int* blocks, int* vec,
                                      int* grid_cap) {
    CTRL_CHECK(blocks && vec && grid_cap, "merge_gather_launch_shape: null argument");
    MergeSlot q[CTRL_MERGE_SLOTS];
    TRY(merge_slots(slots, n_slots, q));
    return merge_gather_launch_shape(q, n_slots, w, R, E, widx_host, K, map, n_in, n_out, in_dtype, out_dtype, blocks, vec, grid_cap);
}
int ctrl_prepare_images(const void* src_u8, int F, int Hin, int Win, const int32_t* hbounds, const int32_t* hk, int hks,
                        const int32_t* vbounds, const int32_t* vk, int vks, void* tmp_u8, void* out, int out_dtype,
                        int W, int H, int repeat, int cfg, void* stream) {
    return op_prepare_images((const unsigned char*)src_u8, F, Hin, Win, hbounds, hk, hks, vbounds, vk, vks, (unsigned char*)tmp_u8,
                             out, out_dtype, W, H, repeat, cfg, S(stream));
}
int ctrl_op_canny_map(const void* src_u8, int N, int H, int W, int C, double low, double high, void* map, void* stream) {
    return op_canny_map((const unsigned char*)src_u8, N, H, W, C, low, high, (unsigned char*)map, S(stream));
}
int ctrl_op_canny_hysteresis(void* map, int N, int H, int W, void* ws, int64_t ws_bytes, int* passes, int* readbacks, void* stream) {
    return op_canny_hysteresis((unsigned char*)map, N, H, W, ws, (long)ws_bytes, passes, readbacks, S(stream));
}
int ctrl_op_canny_finish(const void* map, int N, int H, int W, int out_channels, void* out, void* stream) {
    return op_canny_finish((const unsigned char*)map, N, H, W, out_channels, (unsigned char*)out, S(stream));
}
int ctrl_canny(const void* src_u8, int N, int H, int W, int C, double low, double high, int out_channels, void* out, void* ws,
               int64_t ws_bytes, int* passes, int* readbacks, void* stream) {
    return op_canny((const unsigned char*)src_u8, N, H, W, C, low, high, out_channels, (unsigned char*)out, ws, (long)ws_bytes, passes,
                    readbacks, S(stream));
}
int64_t ctrl_canny_ws_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (double)N * H * W * 3 > 2147483647.0) return 0;      // what every entry above refuses
    return (int64_t)canny_ws_bytes(N, H, W);
}
int ctrl_canny_launch_shape(int H, int W, int* tile_h, int* tile_w) {
    CTRL_CHECK(tile_h && tile_w, "canny_launch_shape: null pointer");
    CTRL_CHECK(H >= 1 && W >= 1, "canny_launch_shape: H and W must be at least 1");
    canny_launch_shape(tile_h, tile_w);
    return 0;
}
}
