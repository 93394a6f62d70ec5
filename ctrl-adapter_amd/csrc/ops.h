// Internal op layer of libctrlhip: every function enqueues hand-written gfx950 kernels on `stream`
// and returns 0 / non-zero (message via ctrl_last_error()).  Activations are fp16, channels-last
// ("NHWC": a feature map [n][y][x][c] is a row-major token matrix [n*H*W][C]); accumulation,
// normalisation statistics, softmax and all epilogue math are fp32.
#pragma once
#include "common.h"
#include "policy.h"
#include "../../include/ctrl_hip.h"

// ------------------------------------------------------------------------------------------
// Implicit GEMM (MFMA f16 -> f32):  out[m][n] = epilogue( sum_k Agather[m][k] * W[n][k] )
// ------------------------------------------------------------------------------------------
// IG_CONV2D_PHASE: a 3x3 conv (padding 1) over a nearest x2 up-sampled map as four 2x2 convs over the source map, one per output
// phase (oy & 1, ox & 1) -- taps = 4, up = 2, W = the phase pack of op_pack_conv_w_phase; see include/ctrl_hip.h: mode
enum { IG_ROWS = 0, IG_CONV2D = 1, IG_TEMPORAL = 2, IG_CONV2D_PHASE = 3 };
enum { SEG_ROW = 0, SEG_TRANSPOSED = 1 };

typedef ctrl_igemm_seg IGemmSeg;     // see include/ctrl_hip.h for field docs
typedef ctrl_igemm_desc IGemmArgs;
int op_igemm(const IGemmArgs& a, hipStream_t s);
// K-split factor op_igemm would use given scratch (1 = no split); scratch needed = factor * M * Nout * sizeof(float)
int igemm_splitk_factor(const IGemmArgs& a);
// scratch bytes for that factor (>= factor * M * Nout * sizeof(float): the in-launch reduction keeps tile-shaped slabs)
size_t igemm_splitk_ws_bytes(const IGemmArgs& a, int sk);
// ticket words (ctrl_igemm_desc::splitk_tickets) the in-launch reduction of `sk` splits uses; 0 = that form does not apply
size_t igemm_splitk_ticket_words(const IGemmArgs& a, int sk);
// tile walk order of the implicit GEMM (tile_order.h): "legacy" | "auto" | "m,G" | "n,G"; 0 = accepted
int igemm_set_order(const char* spec);
// which problems take the 8-phase wide-tile kernel (igemm8_kernel): 0 none, 1 where the grid fills the chip (default), 2 every
// eligible problem (the parity tests run their small shapes through it this way), -1 back to CTRL_IGEMM8 / the default; 0 = accepted
int igemm_set_wide(int mode);
void igemm_tile_of(int bid, int ntm, int ntn, int mode, int group, int* tile_m, int* tile_n);
// what op_igemm (pinned: op_igemm_pinned) would record for `a` as one of group_n same-form problems of a launch: the kernel symbol, then
// " splitkN" for a split problem and " in-launch" where that reduction is taken; launches nothing, needs no device (ctrl_igemm_select)
int igemm_select_text(const IGemmArgs& a, int group_n, bool pinned, char* buf, int cap);
// Grouped launch (round 5): n <= kMaxIGemmGroup problems of the same shape and epilogue form (sibling adapter blocks of one
// pyramid level) in ONE launch -- every problem computed exactly as it would be alone; problems that do not agree are launched one
// by one.  See igemm.hip: IGemmGroup.
constexpr int kMaxIGemmGroup = 4;
constexpr int kMaxGroup = kMaxIGemmGroup;
int op_igemm_group(const IGemmArgs* a, int n, hipStream_t s);
// the same contraction in ONE fixed form whatever M (64 x 64 x 64 tile, no split-K, no grouping): batch-invariant rows (the text encoder)
int op_igemm_pinned(const IGemmArgs& a, hipStream_t s);
// Fused GEGLU feed-forward, dim 512 / hidden 2048 (ffn.hip; include/ctrl_hip.h: ctrl_ffn_desc): one launch instead of the GEGLU GEMM +
// the K = 2048 GEMM; op_ffn_fused deposits into an installed collector like op_igemm does
typedef ctrl_ffn_desc FfnArgs;
bool op_ffn_fused_shape_ok(int dim, int inner);
int op_ffn_fused(const FfnArgs& a, hipStream_t s);
int op_ffn_fused_group(const FfnArgs* a, int n, hipStream_t s);
int op_ffn_pack_w2(const half_t* w2, half_t* out, int N, int K, hipStream_t s);
// convenience: plain linear out[M][N] (fp16 row-major) = A[M][K] * W[N][K]^T + bias
int op_linear(const half_t* A, long lda, const half_t* W, const float* bias, half_t* out, long ldo,
              int M, int N, int K, const half_t* res, long ldres, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Flash attention, one (query tile, head, batch) per workgroup, online softmax in fp32.
//   Q [B*Lq][ldq] (head h at column h*D), K [B*Lk][ldk], Vt [B][heads*D][Lkpad] (V transposed),
//   O [B*Lq][ldo].
// ------------------------------------------------------------------------------------------
typedef ctrl_attn_desc AttnArgs;
int op_flash_attn(const AttnArgs& a, hipStream_t s);
int op_flash_attn_group(const AttnArgs* a, int n, hipStream_t s);      // same-shape problems in one launch (see op_igemm_group)
// Grouped launch of the attention kernels (attention.hip, attention_d64.hip): up to kMaxGroup problems of one shape -- the attentions
// of sibling adapter blocks -- share a launch; the descriptors travel as an array at offset 0 of the kernel-argument segment,
// workgroup b works on problem b / per (per = the workgroups of one problem, a multiple of 8: the XCD of a workgroup stays its local
// index & 7).  A plain launch is a group of one.
struct AttnGroup { AttnArgs a[kMaxGroup]; };
#define ATTN_GROUP_ARGS(gp) (((const AttnArgs*)__builtin_amdgcn_kernarg_segment_ptr())[gp])
// XCD-aware work map of the attention kernels (1-D grid of 8 * ceil(pairs / 8) * qtiles workgroups per problem; workgroup id -> XCD
// id & 7, the observed dispatch order): XCD x owns the whole (batch, head) pairs x, x + 8, ... and walks their query tiles back to back, so the
// workgroups resident on one XCD stream the SAME K / V tiles through that XCD's L2.  Round 6: when pairs is not a multiple of 8 the LAST
// round used to leave 8 - pairs % 8 XCDs without work (B = 2, 5 heads: 10 pairs in 16 slots -- the config-1 step ran its self-attention at 0.29
// of the peak instead of 0.39); the query tiles of those last pairs are now dealt round-robin over all eight XCDs.  false = no work.
#ifdef __HIPCC__
// max of two scores as IEEE-754-2019 maximum (v_maximum3_f32 on gfx950): fmaxf() is maxnum, for which hipcc first QUIETS every operand it has
// not seen produced -- a canonicalising v_max_f32 x, x, x per MFMA output, 5 extra VALU per 64-key tile beside the MFMAs of the attention
// loops (round 6, profiles/r06_attention_pmc.txt).  Same value for every non-NaN input.
#ifdef CTRL_ATTN_FMAXF          // (build.py CTRL_BUILD_FMAXF=1: the rounds 2-5 form, for A/B runs)
__device__ __forceinline__ float vmaxf(float a, float b) { return fmaxf(a, b); }
#else
__device__ __forceinline__ float vmaxf(float a, float b) { return __builtin_elementwise_maximum(a, b); }
#endif
__host__ __device__ __forceinline__ bool attn_work_map(int gbid, int qtiles, int pairs, int* pair, int* qt) {
    const int xcd = gbid & 7, j = gbid >> 3;
    const int full = pairs & ~7;
    const int jr = j - (full >> 3) * qtiles;          // row inside the remainder round (negative before it)
    if (jr < 0) {
        const int r = j / qtiles;
        *pair = r * 8 + xcd;
        *qt = j - r * qtiles;
        return true;
    }
    const int t = jr * 8 + xcd;
    if (t >= (pairs - full) * qtiles) return false;
    const int r = t / qtiles;
    *pair = full + r;
    *qt = t - r * qtiles;
    return true;
}
#endif
// descriptors of the grouped launch being dispatched (op_flash_attn_group); [0] is the problem the dispatcher sees
extern thread_local const AttnArgs* t_attn_grp;
extern thread_local int t_attn_grp_n;
inline int attn_grp_count() { return t_attn_grp ? t_attn_grp_n : 1; }
inline AttnGroup attn_grp_make(const AttnArgs& a) {
    AttnGroup g;
    for (int i = 0; i < attn_grp_count(); ++i) g.a[i] = t_attn_grp ? t_attn_grp[i] : a;
    return g;
}
// instruction-selection variant of the head_dim-64 long-sequence kernel (attention_d64.hip); performance only
int attn_set_variant(int v);

// CLIP text encoder (text.hip): token + position embedding into the fp32 stream fused with the first LayerNorm (fp16 y; ids outside
// [0, V) are clamped and raise *bad), causal self-attention over L <= 128 tokens straight from the [N*L][ld] Q | K | V rows (head_dim 64),
// final LayerNorm into y_dt (+ the pooled row per prompt: argmax(ids) when eos == 2, else the first eos position), fp32 -> y_dt copy
int op_text_embed(const int64_t* ids, const float* tok, const float* pos, int V, int N, int L, int C, float* x,
                  const float* gamma, const float* beta, float eps, half_t* y, int* bad, hipStream_t s);
int op_text_attn(const half_t* qkv, long ld, half_t* out, long ldo, int N, int L, int heads, float scale, hipStream_t s);
int op_text_final(const void* x, int x_dt, int rows, int C, const float* gamma, const float* beta, float eps, void* y, int y_dt,
                  const int64_t* ids, int L, int eos, void* pooled, hipStream_t s);
int op_text_store(const float* x, void* y, int y_dt, size_t n, hipStream_t s);
// op_text_final with C up to 2048 (multiples of 64 above 1024) and the pooled row also in fp32 (pooled32 [N][C], may be null)
int op_text_final_ext(const void* x, int x_dt, int rows, int C, const float* gamma, const float* beta, float eps, void* y, int y_dt,
                      const int64_t* ids, int L, int eos, void* pooled, float* pooled32, hipStream_t s);
// Batch-invariant few-row GEMM (text_gemm.hip): y[M][N] (y_dt) = act(x[M][K] W^T + b) (+ res fp32 [M][N]); act 0 / 2 quick_gelu /
// 3 exact gelu; N % 16 == 0, K % 32 == 0; ws >= text_gemm_ws_bytes(M, N, K) (fp32 split-K partials, reduced in a fixed order)
int text_gemm_splits(int N, int K);
size_t text_gemm_ws_bytes(int M, int N, int K);
int op_text_gemm(const half_t* x, const half_t* W, const float* bias, int M, int N, int K, int act, const float* res, void* y, int y_dt,
                 float* ws, size_t ws_bytes, hipStream_t s);
// y = act(sum of `splits` fp32 planes [M][N] + b) (+ res): the reduction of op_text_gemm (also the unfused activation of a pinned GEMM)
int op_text_gemm_finish(const float* ws, int splits, int M, int N, const float* bias, int act, const float* res, long ldres, void* y,
                        int y_dt, long ldy, hipStream_t s);
// text_embeds[n] = pooled32[n] . Wp^T in fp32 (Wp fp32 [P][C], no bias), out [N][P] in out_dt
int op_text_proj(const float* pooled32, const float* Wp, int N, int C, int P, void* out, int out_dt, hipStream_t s);

// CLIP vision tower (vision.hip): pixels (fp32 / fp16 / bf16 NCHW, or uint8 NHWC / 255) -> im2col rows [N*P][Kpad] fp16, normalised
// (x - mean_c) / std_c in fp32 when mean_std (host, mean[3] | std[3]) is given; [class ; patch rows] + position -> pre_layrnorm (fp32 x)
// -> layer_norm1 (fp16 y); V of the row-major Q | K | V rows -> V^T [N][C][Lkpad] (pad columns zero); post_layernorm of every image's
// row 0 (pooled in y_dt and / or fp32); SVD's _resize_with_antialiasing + (x + 1) / 2 + optional normalise -> [N][3][OH][OW] in out_dt;
// the patch weight [C][K] fp32 -> fp16 [C][Kpad]
int op_vision_patchify(const void* px, int dt, int N, int S, int p, const float* mean_std, half_t* out, int Kpad, hipStream_t s);
int op_vision_embed(const float* patch, const float* cls, const float* pos, int N, int L, int C, const float* g0, const float* b0,
                    const float* g1, const float* b1, float eps, float* x, half_t* y, hipStream_t s);
int op_vision_vt(const half_t* v, long ld, half_t* vt, int N, int L, int C, int Lkpad, hipStream_t s);
int op_vision_cls_ln(const float* x, int N, int L, int C, const float* g, const float* b, float eps, void* pooled, int y_dt, float* pooled32,
                     hipStream_t s);
int op_clip_resize_aa(const void* src, int dt, int N, int H, int W, int OH, int OW, const float* mean_std, void* out, int out_dt, hipStream_t s);
int op_vision_pack_patch(const float* w, int C, int K, int Kpad, half_t* out, hipStream_t s);

// KL-VAE encoder (vae.hip): the mid-block attention's softmax -- P fp16 [rows][ldp] = softmax over the first L columns of the fp32
// scores S [rows][lds], in fp32 (diffusers' upcast_softmax), columns L .. Lpad zeroed; the posterior head -- conv_out rows (NHWC fp32
// [N*h*w][ldx], x_nchw 0) or MOMENTS planes ([N][ldx][h][w], x_nchw 1) -> quant_conv (wq [2lat][2lat] + bq, fp32; NULL = none) ->
// DiagonalGaussianDistribution -> mode / sample / moments NCHW in out_dt (include/ctrl_hip.h: CTRL_VAE_*)
// conv_in of one image: NCHW pixels [3][H][W] (dt) -> fp32 NHWC [H*W][Cout]; w fp32 [9][3][Cout] (op_pack_conv_w_direct), b [Cout]
int op_vae_conv_in(const void* px, int dt, const float* w, const float* b, float* out, int H, int W, int Cout, hipStream_t s);
int op_vae_row_softmax(const float* S, long lds, half_t* P, long ldp, int rows, int L, int Lpad, hipStream_t s);
int op_vae_posterior(const float* x, long ldx, int x_nchw, const float* wq, const float* bq, int N, int lat, int h, int w, const void* eps,
                     int eps_dt, float scale, int kind, void* out, int out_dt, hipStream_t s);

// KL-VAE decoder (vae.hip), one image per call.  Head: NCHW latents [lat][h][w] (dt, ch_stride elements between its dense [h][w] channel
// planes) * scale -> post_quant_conv (wpq fp32 [lat][lat] +
// bpq) -> conv_in 3x3 (w fp32 [9][lat][Cout], op_pack_conv_w_direct) in fp32 -> fp32 NHWC [h*w][Cout].  Tail: fp32 NHWC stream [H*W][C]
// -> conv_norm_out (stats: the sums of op_gn_stats over x) + SiLU -> conv_out 3x3 (w fp32 [9][C][Cout], Cout <= 4) on the VALU in fp32
// -> the epilogue `kind` (include/ctrl_hip.h: CTRL_VAE_DEC_*)
int op_vae_dec_head(const void* z, int dt, float scale, const float* wpq, const float* bpq, const float* w, const float* b, float* out,
                    int lat, int h, int wd, long ch_stride, int Cout, hipStream_t s);
int op_vae_dec_tail(const float* x, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b,
                    int H, int W, int C, int Cout, int kind, void* out, int out_dt, hipStream_t s);
// Temporal decoder (vae.hip): time_conv_out over the frames of one clip.  x fp32 NCHW [F][Cout][H*W] (the tail kernel's SAMPLE / fp32
// frames) -> Conv3d (3,1,1) with zero frames outside [0, F) (w fp32 [Cout][Cout][3] as the checkpoint holds it, b [Cout], Cout <= 4) in
// fp32 -> the epilogue `kind` of the tail kernel over the F frames (NCHW [F][Cout][H][W], or NHWC bytes [F][H][W][Cout])
int op_vae_time_conv(const float* x, const float* w, const float* b, int F, int H, int W, int Cout, int kind, void* out, int out_dt,
                     hipStream_t s);

// temporal attention over the frame axis: tokens X [(b*F+f)*HW + p][...]; seq = F (<= 32)
typedef ctrl_tattn_desc TAttnArgs;
int op_temporal_attn(const TAttnArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Normalisation
// ------------------------------------------------------------------------------------------
// GroupNorm statistics over [img][rows_per_img][C]: stats[img][G][2] = (sum, sumsq), reduced in a fixed order.
// `stats` holds op_gn_stats_floats(...) floats (results first, then tickets and per-workgroup partials) and must have
// been zeroed once (the kernel leaves its tickets zero again).
size_t op_gn_stats_floats(int imgs, int rows_per_img, int C, int G);
// launch shape of the two GroupNorm passes: the launchers aim for about this many workgroups in total (the statistics pass fewer and
// fatter: the last workgroup of an image adds all its chunks).  gn_launch_shape(pass 0 = statistics, 1 = apply) gives rows per
// workgroup and workgroups (chunks) per image exactly as op_gn_stats_group / op_gn_apply_group launch them; host only, false = bad shape
constexpr int kGnStatsBlocks = 768, kGnApplyBlocks = 2048;
bool gn_launch_shape(int imgs, int rows_per_img, int C, int pass, int* rows_per_block, int* chunks);
// ldx: elements between the rows of x (0 = C; larger: x is a column range of wider rows)
int op_gn_stats(const void* x, int x_dtype, float* stats, int imgs, int rows_per_img, int C, int G, hipStream_t s, long ldx = 0);
// y = (x-mean)*rstd*gamma+beta (optionally SiLU); x,y [imgs*rows][C]
// ldy / lo_off: row stride of y (0 = C) and, when > 0, the column offset of the LOW half of a split operand
// (y[r][c] = hi = fp16(v), y[r][lo_off + c] = fp16(v - hi)): consumed by a convolution packed with dup weights
int op_gn_apply(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, half_t* y,
                int imgs, int rows_per_img, int C, int G, float eps, int silu, hipStream_t s, long ldy = 0, int lo_off = 0,
                long stat_rows = 0, long y_img_rows = 0, long y_row0 = 0, long ldx = 0);
//   stat_rows: rows per image the statistics in `stats` span (0 = rows_per_img; larger when a clip's frames are sharded
//   over ranks and the sums were all-reduced); y_img_rows / y_row0: image i of y starts at row i*y_img_rows + y_row0
//   (0 = dense): the padded operand layout of the frame-sharded temporal convolution
// LayerNorm over the last dim of x [M][C] -> y fp16
int op_layernorm(const void* x, int x_dtype, long ldx, const float* gamma, const float* beta, half_t* y, long ldy,
                 int M, int C, float eps, hipStream_t s);
// xsum[m][c] = x[m][c] + addv[((m / rows_per_img) % vmod) * ldv + c] (in x's dtype, row stride ldx) and y = LayerNorm(xsum):
// the frame-index embedding add in front of the temporal transformer and its first LayerNorm in one pass
int op_layernorm_add(const void* x, int x_dtype, long ldx, const float* addv, long ldv, int rows_per_img, int vmod, void* xsum,
                     const float* gamma, const float* beta, half_t* y, long ldy, int M, int C, float eps, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Element-wise / layout / small kernels
// ------------------------------------------------------------------------------------------
// [N][C][HW] (any dtype) -> [N][HW][C] fp16
int op_nchw_to_nhwc(const void* x, int dtype, half_t* y, int N, int C, int HW, hipStream_t s);
// [N][HW][C] fp16 -> [N][C][HW] (any dtype), y = x*scale
int op_nhwc_to_nchw(const half_t* x, void* y, int dtype, int N, int C, int HW, float scale, hipStream_t s,
                    const int* img_map = nullptr);   // img_map (device): image n is written at image img_map[n]
// exact kxk mean pooling of an NCHW tensor (adaptive_avg_pool2d with integer ratio), dtype preserved
int op_avgpool_nchw(const void* x, void* y, int dtype, int NC, int Hin, int Win, int Hout, int Wout, hipStream_t s);
// sinusoidal timestep embedding, flip_sin_to_cos=True, shift 0: out[n][dim] fp32 = [cos | sin]
int op_timestep_sincos(const float* t, int t_count, float* out, int N, int dim, hipStream_t s);
// frame-index variant: t[n] = n % F
int op_frameidx_sincos(float* out, int N, int F, int dim, hipStream_t s);
// small-M linear (M <= 64): out[m][n] = act(sum_k in_act(x[m][k]) * w[n][k] + b[n]); x,out fp32; w fp16
//   in_silu: apply SiLU to x on load; out_silu: apply SiLU to the result
int op_linear_small(const float* x, long ldx, const half_t* w, const float* b, float* out, long ldo,
                    int M, int N, int K, int in_silu, int out_silu, hipStream_t s);
// grouped form: `count` independent small-M linears, kSmallGroup per launch
struct SmallLin { const float* x; long ldx; const half_t* w; const float* b; float* out; long ldo; int M, N, K, in_silu, out_silu; };
constexpr int kSmallGroup = 40;
struct SmallLinGroup { SmallLin p[kSmallGroup]; int blk_begin[kSmallGroup]; int count; };
int op_linear_small_group(const SmallLin* probs, int count, hipStream_t s);
// y[m][c] = a*x1[m][c] + b*x2[m][c]   (AlphaBlender; a=alpha, b=1-alpha read from device: alpha=sigmoid(*mix))
int op_blend(const void* x_spatial, int xs_dt, const void* x_temporal, int xt_dt, const float* mix_factor, void* y, int y_dt, size_t n, hipStream_t s);
// y[m][c] = x[m][c] + v[(m / rows_per_img) % vmod][c]   (fp32 per-image vector broadcast add)
int op_add_rowvec(const void* x, int x_dt, const float* v, long ldv, void* y, int y_dt, size_t M, int C, int rows_per_img, int vmod, hipStream_t s);
// rows (clip, frame, pixel): y = x + v[(b*L + p) % B]  (per-clip time context of the temporal transformer, see the kernel)
int op_add_rowvec_clip(const void* x, int x_dt, const float* v, long ldv, void* y, int y_dt, int B, int F, int L, int C, hipStream_t s);
// nearest x2 up-sampling of an NHWC fp16 map
int op_upsample2x_nhwc(const half_t* x, half_t* y, int N, int H, int W, int C, hipStream_t s);
// fill fp16/any
int op_fill_zero(void* p, size_t bytes, hipStream_t s);
int op_fill_zero_group(void* const* p, const size_t* bytes, int n, hipStream_t s);      // up to kMaxGroup fills in one launch
// K-way weighted merge of NCHW tensors: out = sum_e w[widx[e]] * x_e   (router merge; weights on device)
int op_weighted_merge(const void* const* xs_dev, const float* w, const int* widx_dev, int K, void* out, int dtype,
                      size_t n, hipStream_t s);
// router merge + key-frame gather + cast of up to 13 slots in ONE launch: out[s][j] = sum_k w[row_s E + widx[k]] in_k[s][map[j]], frames of
// `elems` elements; map (device int32 [n_out], NULL = identity) indexes the n_in input frames; w NULL (K == 1) = weight 1, an exact gather.
// The slot table travels in the kernel arguments: no host access to device memory, no synchronisation, capturable.
struct MergeSlot { const void* in[8]; void* out; long elems; int row; };
int op_merge_gather_group(const MergeSlot* slots, int n_slots, const float* w, int R, int E, const int* widx, int K, const int* map, int n_in,
                          int n_out, int in_dt, int out_dt, hipStream_t s);
// how that launch would run: workgroups, elements per thread and access (8 | 1), the grid cap (host only; the same checks)
int merge_gather_launch_shape(const MergeSlot* slots, int n_slots, const float* w, int R, int E, const int* widx, int K, const int* map,
                              int n_in, int n_out, int in_dt, int out_dt, int* blocks, int* vec, int* grid_cap);
// router: weights[r][e] = softmax_e( wg[r][e] (or 0) - 1e6*(1-mask[e]) ),  r in [0,R)
int op_router_softmax(const float* wg, const int* mask, float* out, int R, int E, int equal_weights, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Direct 3x3 convolution for tiny channel counts (ControlNet stem / conditioning embedder head)
//   in : NCHW any dtype (in_nchw=1) or NHWC fp16;  w fp32 [9][Cin][Cout]; out NHWC fp16 (+bias, optional SiLU)
// ------------------------------------------------------------------------------------------
int op_conv3x3_direct(const void* in, int in_dtype, int in_nchw, const float* w, const float* bias, half_t* out,
                      int N, int Cin, int Cout, int Hin, int Win, int stride, int silu, hipStream_t s);

// the UNets' stems (Cin = 8: SVD, Cin = 4: SDXL): NCHW sample of any dtype -> fp32 NHWC rows (the residual stream), stride 1, no activation
int op_conv3x3_direct_f32(const void* in, int in_dtype, const float* w, const float* bias, float* out, int N, int Cin, int Cout, int H,
                          int W, hipStream_t s);

// the I2VGen-XL UNet's stem: channels-last fp32 operand rows [N*H*W][8] (sample | encoded image latents) -> fp32 NHWC rows
int op_conv3x3_rows_f32(const float* in, const float* w, const float* bias, float* out, int N, int Cin, int Cout, int H, int W, hipStream_t s);

// The same convolution on the matrix cores for the channels-last layers with Cin, Cout in {16, 32} (the conditioning embedder's
// 16 -> 16, 16 -> 32 s2, 32 -> 32): x NHWC fp16, w fp16 [Cout][9][Cin] (op_pack_conv_w), out NHWC fp16 (+ bias, optional SiLU)
bool op_conv3x3_small_mfma_applies(int Cin, int Cout);
int op_conv3x3_small_mfma(const half_t* x, const half_t* w, const float* bias, half_t* out, int N, int Cin, int Cout, int Hin, int Win,
                          int stride, int silu, hipStream_t s);

// weight packing (load time)
// conv weight [Cout][Cin][kh][kw] (any dtype) -> fp16 [Cout][kh*kw][Cin]   (taps-major K)
int op_pack_conv_w(const void* w, int dtype, half_t* out, int Cout, int Cin, int taps, hipStream_t s, int* ovf = nullptr);
//   ovf (optional, device): set to 1 when a value does not fit fp16 (|w| > 65504, inf, nan)
// split-operand form: fp16 [Cout][taps][2*Cin], the Cin weights of every tap twice
int op_pack_conv_w_dup(const void* w, int dtype, half_t* out, int Cout, int Cin, int taps, hipStream_t s, int* ovf = nullptr);
// phase form of a 3x3 conv over a nearest x2 up-sampled map (IG_CONV2D_PHASE): [Cout][Cin][3][3] -> fp16 [4 phases][Cout][4 taps][Cin];
// phase (a, b) = (oy & 1, ox & 1), tap (ty, tx) = the sum of the 3x3 weights whose window row / column falls on source row
// i + a - 1 + ty / column j + b - 1 + tx: rows {0} | {1, 2} for a = 0, {0, 1} | {2} for a = 1.  Summed in fp32, rounded once
int op_pack_conv_w_phase(const void* w, int dtype, half_t* out, int Cout, int Cin, hipStream_t s, int* ovf = nullptr);
// conv weight [Cout][Cin][3][3] -> fp32 [9][Cin][Cout] for the direct kernel
int op_pack_conv_w_direct(const void* w, int dtype, float* out, int Cout, int Cin, hipStream_t s);
// linear weight [N][K] -> fp16 [N][K]; optional GEGLU interleave of rows (N = 2*inner)
int op_pack_linear_w(const void* w, int dtype, half_t* out, int N, int K, int geglu, hipStream_t s, int* ovf = nullptr);
// vector -> fp32 (optional GEGLU interleave)
int op_pack_vec(const void* v, int dtype, float* out, int N, int geglu, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Backbone UNets: SVD and SDXL (unet.hip)
// ------------------------------------------------------------------------------------------
// one skip tensor of the up path: out[r][col + c] = skip[r][c] (+ res(b, f, c, p)) for the B * F * HW rows r = (b F + f) HW + p and
// c < C2, the fp32 master (row stride ld_out) and, when out16 is given, its fp16 mirror with one rounding.  res (optional): the adapter's
// residual as the caller holds it, (b f) c h w (res_5d = 0) or b c f h w (res_5d = 1), fp32 / fp16 / bf16.  skip may alias out32
// (the mid residual, col = 0, added in place).
// lo_off > 0: the mirror is a split [hi | lo] row pair -- rows 2 * ld_out halves apart, lo = fp16(x - hi) at column lo_off + col + c
int op_unet_skip_join(const float* skip, long ld_skip, const void* res, int res_dt, int res_5d, int B, int F, int HW, int C2, float* out32,
                      half_t* out16, long ld_out, int col, hipStream_t s, int lo_off = 0);
// conv_out: x fp16 NHWC [N][H][W][C] (normalised + activated), w fp32 [9][C][Cout] (op_pack_conv_w_direct), Cout <= 4 -> NCHW out_dt
// layout: where image n lands -- CONV_OUT_NCHW [N][Cout][H][W] (the default), CONV_OUT_NCFHW [N / frames][Cout][frames][H][W] (the
// I2VGen-XL UNet's b c f h w output, image n = (b, f)), CONV_OUT_ROWS channels-last rows [N * H * W][Cout] (its 16 -> 4 latent stem)
enum { CONV_OUT_NCHW = 0, CONV_OUT_NCFHW = 1, CONV_OUT_ROWS = 2 };
int op_unet_conv_out(const half_t* x, const float* w, const float* bias, void* out, int out_dt, int N, int H, int W, int C, int Cout,
                     hipStream_t s, int layout = CONV_OUT_NCHW, int frames = 1);

// I2VGen-XL's backbone UNet (unet.hip).  image_latents [B][4][F][HW] (fp32 / fp16 / bf16) -> fp32 planes [(b f)][4][HW]
int op_i2v_frames(const void* x, int dt, float* y, int B, int F, int HW, hipStream_t s);
// I2VGenXLTransformerTemporalEncoder (dim 4, two heads of 4, FF 4 -> 16 -> 4, erf GELU) over the F <= 32 frames of every pixel, fp32:
// x rows [(b f) HW][4] (image_latents_proj_in's output) -> columns 4..7 of the conv_in operand rows out8 [(b f) HW][8]; sample
// (optional, [B][4][F][HW] in sample_dt) -> columns 0..3; keep (optional) [(b f) HW][4]: the encoded latents once more.
// wts (288 floats): ln g[4] b[4] | to_q [8][4] | to_k [8][4] | to_v [8][4] | to_out [4][8] b[4] | ff.net.0.proj [16][4] b[16] | ff.net.2 [4][16] b[4]
// precomputed = 1: x already holds encoded latents (a kept forward's `keep`), which are copied
int op_i2v_latent_encoder(const float* x, const float* wts, const void* sample, int sample_dt, float* out8, float* keep, int B, int F,
                          int HW, int precomputed, hipStream_t s);
// adaptive_avg_pool2d of a channels-last map [N][H][W][C] (fp32 | fp16) to [N][OH][OW][C] (fp32 | fp16): windows
// [floor(i H / OH), ceil((i + 1) H / OH)), summed in fp32; replication where H < OH
int op_adaptive_avgpool_nhwc(const void* x, int x_dt, void* y, int y_dt, int N, int H, int W, int C, int OH, int OW, hipStream_t s);

// the operand rows of add_embedding.linear_1 of a text_time UNet (SDXL): out fp32 [B][ld_out], columns [0, text_dim) = text_embeds[b]
// (fp32 / fp16 / bf16) converted, columns text_dim + i * dim + [0, dim) = [cos | sin] of time_ids[b][i] (sincos_kernel's arithmetic)
int op_unet_text_time(const void* text, int text_dt, int text_dim, const float* ids, int n_ids, int dim, float* out, long ld_out, int B,
                      hipStream_t s);

// ------------------------------------------------------------------------------------------
// Samplers (sampler.hip): the per-step glue of a denoise loop as one streaming launch.  See include/ctrl_hip.h: ctrl_sampler_desc.
//   with_step: prev = A_i x + B_i (u + g (c - u));  with_input: the model's inputs (c_in scaling, CFG replicas, concat, the ControlNet's
//   sample, the three timestep scalars) of row i (alone) or of row i + 1 from the rounded prev (after a step; skipped past the table).
//   step_index < 0: i is counter[0]; a launch with a step then advances it by a ticket (counter[1]): the last workgroup to finish.
// ------------------------------------------------------------------------------------------
typedef ctrl_sampler_desc SamplerDesc;
constexpr int kSamplerGridCap = 1024;
int op_sampler(const float* table, int n_steps, int* counter, float* scalars, const SamplerDesc& d, int step_index, bool with_step,
               bool with_input, hipStream_t s);
int op_sampler_reset(int* counter, hipStream_t s);
// validation + launch shape of the above (host only): workgroups, elements per access (8 | 1)
int sampler_launch_shape(const SamplerDesc& d, bool with_step, bool with_input, int* blocks, int* vec);

// ------------------------------------------------------------------------------------------
// Conditioning-image preparation (model/ctrl_helper.py:268-296): Pillow-exact 8-bit Lanczos resize + /255 + NCHW + repeats
//   src uint8 [F][Hin][Win][3]; h/v bounds int32 [out][2] + weights int32 [out][ks] (null = axis not resampled);
//   tmp uint8 [F][Hin][W][3] (horizontal pass result); out [cfg][rep*F][3][H][W] in out_dtype
// ------------------------------------------------------------------------------------------
int op_prepare_images(const unsigned char* src, int F, int Hin, int Win, const int* hbounds, const int* hk, int hks,
                      const int* vbounds, const int* vk, int vks, unsigned char* tmp, void* out, int out_dtype,
                      int W, int H, int rep, int cfg, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Canny condition extraction (model/ctrl_helper.py:171-179), cv2.Canny(img, low, high) bit for bit (canny.hip):
//   src uint8 [N][H][W][C], C = 1 | 3 -> map uint8 [N][H][W] (0 none, 1 weak, 2 strong) -> hysteresis in place, pass by pass until a
//   pass promotes nothing (reads a flag back: not capturable) -> out uint8 [N][H][W] | [N][H][W][3] of 0 / 255.
//   ws: canny_ws_bytes(N, H, W) for op_canny (flag block + map); op_canny_hysteresis alone needs the 256-byte flag block.
//   *passes = passes up to and including the first that promoted nothing, *readbacks = flag readbacks (host synchronisations).
// ------------------------------------------------------------------------------------------
void canny_launch_shape(int* tile_h, int* tile_w);
long canny_ws_bytes(int N, int H, int W);
int op_canny_map(const unsigned char* src, int N, int H, int W, int C, double low, double high, unsigned char* map, hipStream_t s);
int op_canny_hysteresis(unsigned char* map, int N, int H, int W, void* ws, long ws_bytes, int* passes, int* readbacks, hipStream_t s);
int op_canny_finish(const unsigned char* map, int N, int H, int W, int out_channels, unsigned char* out, hipStream_t s);
int op_canny(const unsigned char* src, int N, int H, int W, int C, double low, double high, int out_channels, unsigned char* out,
             void* ws, long ws_bytes, int* passes, int* readbacks, hipStream_t s);

// ------------------------------------------------------------------------------------------
// HED annotator (hed.hip; controlnet_aux HEDdetector: the `scribble` branch of model/ctrl_helper.py:196-197 and the soft-edge condition)
//   stem: src uint8 [N][H][W][3] -> relu(conv3x3((x - norm3) * scale) + bias) fp16 [N][H][W][64]; w fp32 [9][3][64]
//   (op_pack_conv_w_direct), bias [64] (already multiplied by scale), norm3 on the HOST; nonfinite (optional): raised when a value leaves fp16
//   pool_proj: h fp16 [N][H][W][C] -> p fp32 [N][H][W] = inv_scale * (h . wp) + bp[0] and, when pooled is given, max_pool2d(2, 2) of h
//   fuse: maps5 (host array of five device maps, fp32 [N][H >> k][W >> k]) -> cv2 INTER_LINEAR to H x W, mean (logits, optional fp32
//   [N][H][W]), sigmoid, * 255, clip, truncate -> uint8 [N][H][W] | [N][H][W][3]
//   blur_f32 / nms / blur_u8_bin: the scribble tail at sigma 3 (25 taps to fp32; threshold 127; 19 taps to uint8, > 4 -> 255 else 0),
//   bit for bit tests/hed_ref.py
// ------------------------------------------------------------------------------------------
int op_hed_stem(const unsigned char* src, int N, int H, int W, const float* w, const float* bias, const float* norm3, float scale, half_t* out,
                int32_t* nonfinite, hipStream_t s);
int op_hed_pool_proj(const half_t* h, int N, int H, int W, int C, const float* wp, const float* bp, float inv_scale, half_t* pooled, float* p,
                     hipStream_t s);
int op_hed_fuse(const float* const* maps5, int N, int H, int W, int out_channels, unsigned char* out, float* logits, hipStream_t s);
int op_hed_blur_f32(const unsigned char* src, int N, int H, int W, float* out, hipStream_t s);
int op_hed_nms(const float* x, int N, int H, int W, unsigned char* out, hipStream_t s);
int op_hed_blur_u8_bin(const unsigned char* src, int N, int H, int W, int out_channels, unsigned char* out, hipStream_t s);
int op_hed_scale_vec(float* v, int n, float scale, hipStream_t s);

// ------------------------------------------------------------------------------------------
// PiDiNet annotator (pidinet.hip; controlnet_aux PidiNetDetector: the `softedge` branch of model/ctrl_helper.py:103-107, 184-185).
// Layouts and semantics: include/ctrl_hip.h (ctrl_op_pidi_*).  fp16 NHWC activations, channels padded to a multiple of 64 (pidi_cp).
// ------------------------------------------------------------------------------------------
inline int pidi_cp(int C) { return (C + 63) & ~63; }
constexpr int kPidiHeadC = 24, kPidiHeadCP = 32, kPidiHeadTaps = 36;
void pidi_launch_shape(int kernel, int* tile_h, int* tile_w);
int pidi_convert_pdc(int kind, const float* w, int Co, int Ci, float* out);      // host only
int op_pidi_stem(const unsigned char* src, int N, int H, int W, const float* w, half_t* out, int32_t* nonfinite, hipStream_t s);
int op_pidi_block(const half_t* x, int N, int H, int W, int Cin, int Cout, int taps, const float* dw, const half_t* w2, const half_t* wsc,
                  const float* bsc, int pool, half_t* out, int32_t* nonfinite, hipStream_t s);
int op_pidi_head_reduce(const half_t* x, int N, int H, int W, int C, const half_t* w1, const float* b1, half_t* t, int32_t* nonfinite,
                        hipStream_t s);
int op_pidi_head_context(const half_t* t, int N, int H, int W, const half_t* wd, const float* par124, float* a4, float* d, hipStream_t s);
int op_pidi_side(const float* a4, const float* d, int N, int H, int W, const float* par37, float* e, hipStream_t s);
int op_pidi_fuse(const float* const* maps4, int N, int H, int W, const float* par5, int apply_filter, int out_channels, unsigned char* out,
                 float* logits, hipStream_t s);

// ------------------------------------------------------------------------------------------
// Lineart annotator (lineart.hip; controlnet_aux LineartDetector: the `lineart` branch of model/ctrl_helper.py:111-114, 190-191).
// Layouts and semantics: include/ctrl_hip.h (ctrl_op_lineart_*, ctrl_op_in_*).
// ------------------------------------------------------------------------------------------
// kernel 0 stem / 1 head: the output tile (rows, columns) of one workgroup; 2: rows of an image one workgroup of in_stats reduces (C given), 1
void lineart_launch_shape(int kernel, int C, int* a, int* b);
int op_lineart_stem(const unsigned char* src, int N, int H, int W, const float* w, half_t* out, int32_t* nonfinite, hipStream_t s);
// floats of scratch op_in_stats needs (the per-workgroup partials); 0 = a shape it refuses
size_t op_in_stats_ws_floats(int N, int HW, int C);
int op_in_stats(const half_t* x, int N, int HW, int C, float* stats, float* ws, hipStream_t s);
int op_in_apply(const half_t* x, const float* stats, int N, int H, int W, int C, float eps, int relu, const half_t* res, int res_pad, int pad,
                half_t* out, int32_t* nonfinite, hipStream_t s);
int op_lineart_head(const half_t* xp, int N, int H, int W, const float* w, float bias, int out_channels, unsigned char* out, float* logits,
                    hipStream_t s);
// ConvTranspose2d(3, stride 2, padding 1, output_padding 1) weight [Cin][Cout][3][3] -> the phase pack fp16 [4][Cout][4][Cin] (IG_CONV2D_PHASE)
int op_pack_convT_w_phase(const void* w, int dtype, half_t* out, int Cin, int Cout, hipStream_t s, int* ovf = nullptr);

// ------------------------------------------------------------------------------------------
// Grouped launches over sibling problems (round 5). The adapter blocks of one pyramid level are independent and have identical
// shapes (model/ctrl_adapter.py:181-191 simply runs them one after the other): the plan records the op sequence of every sibling and
// replays the sequences in lock-step; while a collector is installed, the ops below deposit their arguments instead of launching,
// and flush() launches what was deposited for one step -- as ONE grouped launch when the problems agree in shape and form,
// one by one otherwise.  Every problem is computed exactly as it would be alone: results are bit-identical to the ungrouped forward.
// ------------------------------------------------------------------------------------------
struct GnStatsArgs { const void* x; int x_dtype; float* stats; int imgs, rows_per_img, C, G; long ldx; };
struct GnApplyArgs { const void* x; int x_dtype; const float* stats; const float* gamma; const float* beta; half_t* y;
                     int imgs, rows_per_img, C, G; float eps; int silu; long ldy; int lo_off; long stat_rows, y_img_rows, y_row0, ldx; };
struct LnArgs { const void* x; int x_dtype; long ldx; const float* addv; long ldv; int rows_per_img, vmod; void* xsum;
                const float* gamma; const float* beta; half_t* y; long ldy; int M, C; float eps; };
int op_gn_stats_group(const GnStatsArgs* a, int n, hipStream_t s);
int op_gn_apply_group(const GnApplyArgs* a, int n, hipStream_t s);
int op_layernorm_group(const LnArgs* a, int n, hipStream_t s);
// GroupNorm(32) of a SMALL map (the 80-channel slice of one image <= 512 KB) in ONE launch: statistics + apply by the same workgroup
// (norm.hip: gn_fused_kernel); op_gn_fused_applies says whether the plans use it for a problem (only with CTRL_GN_FUSED=1: measured
// slower than the two-kernel form in the step) -- op_gn_fused itself takes every small map
bool op_gn_fused_fits(int x_dtype, int rows_per_img, int C, int G);
bool op_gn_fused_applies(int x_dtype, int rows_per_img, int C, int G);
int op_gn_fused(const void* x, int x_dtype, const float* gamma, const float* beta, half_t* y, int imgs, int rows_per_img, int C, int G,
                float eps, int silu, hipStream_t s, long ldy = 0, int lo_off = 0);
int op_gn_fused_group(const GnApplyArgs* a, int n, hipStream_t s);

struct OpCollector {
    enum { NONE = 0, IGEMM, GN_STATS, GN_APPLY, LAYERNORM, ATTN, GN_FUSED, FILL, FFN };
    int type = NONE, n = 0;
    hipStream_t s = nullptr;
    IGemmArgs ig[kMaxGroup];
    GnStatsArgs gs[kMaxGroup];
    GnApplyArgs ga[kMaxGroup];
    LnArgs ln[kMaxGroup];
    AttnArgs at[kMaxGroup];
    FfnArgs ff[kMaxGroup];
    struct Fill { void* p; size_t bytes; } fz[kMaxGroup];
    // make room for one more problem of `type` on stream `s` (flushes what is pending when it cannot join); returns its index or -1
    int slot(int type_, hipStream_t s_, int* rc);
    int flush();
};
extern thread_local OpCollector* t_collect;
// CTRL_GROUP=0 turns grouped launches off (every problem in its own launch, as in rounds 1-4); 2 keeps them but lets the GEMM
// dispatcher choose the tile as if every problem ran alone (then results are bit-identical to the ungrouped forward: the tests)
bool group_launches_enabled();
bool group_tiles_as_alone();
