/* libctrlhip -- C ABI of the MI355X-native (gfx950) Ctrl-Adapter denoising hot path.
 *
 * Drop-in boundary for the per-timestep ControlNet forward + Ctrl-Adapter forward (+ router / merge) of
 * HL-hanlin/Ctrl-Adapter.  Every entry point takes plain device pointers and sizes (no torch types),
 * enqueues hand-written HIP kernels on the caller's stream (`stream` is a hipStream_t passed as void*;
 * NULL = default stream), never synchronises, and returns 0 on success / non-zero on error with the
 * message available from ctrl_last_error().  No C++ exception crosses this boundary.
 *
 * Plan-level entry points (what a reference-side binding calls):
 *   ctrl_controlnet_forward   replaces ControlNetModel.forward            controlnet/controlnet.py:662-881
 *   ctrl_adapter_forward      replaces ControlNetAdapter.forward          model/ctrl_adapter.py:171-224
 *                             (and AdapterSpatioTemporal.forward          model/adapter_spatial_temporal.py:175-292,
 *                              ResnetBlock2D.forward                      model/resnet_block_2d.py:164-221)
 *   ctrl_router_weights       replaces ControlNetRouter.forward           model/ctrl_router.py:85-112
 *   ctrl_router_merge         replaces the caller-side expert merge       i2vgen_xl/pipelines/
 *                             i2vgen_xl_controlnet_adapter_pipeline.py:1000-1022 (and train.py:1262-1276)
 *   ctrl_avgpool_nchw         replaces F.adaptive_avg_pool2d(latents,(64,64))  sdxl/pipelines/
 *                             sdxl_controlnet_adapter_pipeline.py:1306-1309
 *   ctrl_text_encoder_forward replaces the CLIPTextModel call of ControlNetHelper.encode_controlnet_prompt
 *                             model/ctrl_helper.py:300-457 (SD-1.5's CLIP ViT-L/14 text tower)
 *   ctrl_text_encoder_forward_ext  replaces the two text-tower calls of the SDXL pipeline's encode_prompt
 *                             sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:282-515 (CLIP ViT-L and OpenCLIP ViT-bigG with
 *                             its text_projection)
 *   ctrl_vision_encoder_forward replaces the image_encoder call of the SVD / I2VGen-XL pipelines' _encode_image
 *                             svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212, i2vgen_xl/...:366-396 (CLIP ViT-H/14)
 * Op-level entry points (ctrl_op_*) expose the individual kernels for parity tests and micro-benchmarks.
 */
#ifndef CTRL_HIP_H
#define CTRL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTRL_ABI_VERSION 11

/* element types of boundary tensors */
enum { CTRL_F32 = 0, CTRL_F16 = 1, CTRL_BF16 = 2 };

/* ---------------------------------------------------------------- runtime */
int ctrl_abi_version(void);
const char* ctrl_last_error(void);           /* thread-local, valid until the next failing call */
/* per-kernel-class HIP-event profiler: begin -> run forwards -> end(sync) -> query */
int ctrl_prof_begin(void);
int ctrl_prof_end(void);
int ctrl_prof_count(void);
/* flops / bytes: ALGORITHMIC work summed over the class's launches (2*M*N*K, 4*B*h*Lq*Lk*D, one read + one write, ...) */
int ctrl_prof_get(int i, char* name, int name_len, double* total_ms, int* launches, double* flops, double* bytes);
/* per-launch records of the last finished profile, in launch order: kernel class tag, kernel symbol with template
   arguments (as rocprofv3 prints it), shape note, HIP-event time on the launch stream, algorithmic work, grid size in
   work-items (= rocprofv3's Grid_Size, which tells the shapes of one symbol apart) */
int ctrl_prof_launch_count(void);
int ctrl_prof_launch_get(int i, char* tag, int tag_len, char* symbol, int symbol_len, char* detail, int detail_len,
                         double* ms, double* flops, double* bytes, int64_t* grid_threads);

/* ---------------------------------------------------------------- op level */
typedef struct ctrl_igemm_seg {
    void* out;          /* destination */
    int64_t ld;         /* ROW: row stride (elements); TRANSPOSED: padded token stride */
    int32_t col_begin;  /* first output column of the segment (multiple of 16) */
    int32_t ncols;      /* segment width */
    int32_t fmt;        /* 0 ROW: out[m*ld + c];  1 TRANSPOSED: out[((m/L)*ncols + c)*ld + m%L] */
    int32_t dtype;      /* CTRL_F32 / CTRL_F16 / CTRL_BF16 */
    int32_t L;          /* tokens per image (TRANSPOSED) */
    int32_t pad_;
    const int32_t* img_map;   /* TRANSPOSED, optional (device): image m/L is written at image img_map[m/L] (frame scatter) */
} ctrl_igemm_seg;

typedef struct ctrl_igemm_desc {
    const void* A;      /* fp16 activations, channels-last */
    int64_t lda;        /* elements between consecutive pixels/rows */
    int32_t mode;       /* 0 rows (linear / 1x1), 1 conv2d, 2 temporal (3 frame taps), 3 conv2d in PHASE form: a 3x3 conv (padding 1)
                           over a nearest x2 up-sampled map, computed as four 2x2 convs over the SOURCE map, one per output phase
                           (oy & 1, ox & 1) -- 4/9 of the FLOPs.  taps = 4, up = 2, stride = 1, tap_origin = 0, Hin / Win = the source
                           grid, Hout = 2 Hin, Wout = 2 Win, M = images * Hout * Wout, Ktot = 4 * Cin, W = the phase pack
                           fp16 [4][Nout][4][Cin] of ctrl_op_pack_conv_w_phase.  Row-major outputs only; no residual, GEGLU, blend,
                           split operand or split-K; Cin % 64 == 0 */
    int32_t Cin;        /* K per tap */
    int32_t taps;       /* 1 | 9 | 3 (temporal) | 4 (phase form) */
    int32_t Hin, Win, Hout, Wout, stride, up;   /* conv2d geometry; up = nearest up-sampling folded into the gather */
    int32_t F, HW;      /* temporal: frames per clip, rows per frame */
    int32_t t_pad;      /* temporal, frame-sharded clip: A = padded [clip][F+2][HW][lda] (slots 0 / F+1 = halo frames), M rows = the F local frames */
    const void* W;      /* fp16 [Nout][taps*Cin] */
    int32_t M, Nout, Ktot;
    int32_t tap_origin; /* conv2d 3x3: 0 = taps at stride*o - 1 .. stride*o + 1 (padding 1 on every side); 1 = taps at stride*o ..
                           stride*o + 2 (no padding before the map, zeros past its end: diffusers' Downsample2D(padding=0) after
                           F.pad(x, (0, 1, 0, 1))) */
    const float* bias;  /* [Nout] or NULL */
    const float* rowvec; int32_t rowvec_ld; int32_t rows_per_img;   /* + rowvec[(m/rows_per_img)*ld + n] */
    const void* res; int64_t ldres;                                 /* + res[m*ldres + n] (fp16, or fp32 if res_f32) */
    float scale;
    int32_t geglu;      /* weights packed in interleaved (hidden,gate) 16-column blocks; out width Nout/2 */
    int32_t nseg;
    int32_t act;        /* 0 none, 1 SiLU, 2 quick_gelu x*sigmoid(1.702x) (CLIP's MLP), 3 ReLU (the HED trunk: a negative value becomes
                           a zero, a value of at least 2^-120 is kept bit for bit); applied after bias/rowvec (before residual) */
    int32_t res_f32;    /* residual is fp32 (the fp32 residual stream) */
    int32_t a_split;    /* split operand: A rows hold [hi | lo] fp16 halves of an fp32 operand along Cin (lo = fp16(x - hi)), so the
                           product is exact in A to ~2^-22 at twice the MFMA work (the ControlNet's convolutions).
                           1: W = every tap's Cin/2 weights packed twice ([Cout][taps][Cin]), K walked as one long axis;
                           2: W = the plain pack [Cout][taps][Cin/2]; k-tiles alternate hi / lo chunk of the same channels and
                              each weight tile is staged once per pair (Cin/2 % 64 == 0) */
    void* splitk_ws; int64_t splitk_ws_bytes;   /* optional fp32 scratch: enables split-K for small-M / long-K problems */
    int32_t* splitk_tickets;   /* optional (device): ZEROED ticket words for the in-launch reduction -- one per 256-row output tile for 2..4 splits, five per tile
                                  for the two-level reduction of 5..16 splits (ctrl-adapter_amd/csrc/igemm.hip: igemm_splitk_ticket_words) (the
                                  plans hand out slices of a pool they zero once per forward); NULL = the library zeroes ticket words
                                  at the end of splitk_ws with a fill launch of its own */
    void* out16; int64_t ld16;   /* optional fp16 row-major mirror of the (single, row-major) output: GEMM-operand copy of an fp32 stream */
    /* optional AlphaBlender fold (diffusers AlphaBlender, model/adapter_spatial_temporal.py:229,282), row-major outputs
     * only: out = (1-a) * y + a * blend_x[m*ld_blend + n], a = sigmoid(*blend_mix), y = the epilogue result above */
    const float* blend_mix; const void* blend_x; int64_t ld_blend; int32_t blend_f32;
    int32_t out16_lo_off;   /* > 0: the fp16 mirror is a split operand, out16[m*ld16 + n] = hi, out16[m*ld16 + out16_lo_off + n] = lo */
    float scale2; int32_t scale2_from;   /* scale2_from > 0: output columns scale2_from <= n < scale2_to are multiplied by scale2 instead
                                            of scale: the K third of a Q|K|V projection leaves pre-multiplied by
                                            softmax_scale * log2(e) for ctrl_attn_desc::k_prescaled */
    int32_t res_up;     /* 2: conv2d only -- `res` holds [img][Hout/2][Wout/2][ldres] and is read through a nearest x2 up-sampling
                           (res[img][oy/2][ox/2]); 0 | 1: res[m*ldres + n] */
    int32_t scale2_to;  /* end of the scale2 column range (0 = Nout) */
    /* Output segments (1..3, ascending col_begin).  Mixed layouts -- row-major segments followed by ONE transposed last segment,
       the Q | K | V^T outputs of a self-attention projection in one launch -- run on the vector epilogue when the transposed
       segment starts at a multiple of 64 columns (the dispatcher then only picks tiles whose width divides that boundary, so
       every tile lies in one segment); anything else takes the scalar epilogue. */
    ctrl_igemm_seg seg[3];
    int32_t* nonfinite;  /* optional (device): set to 1 when an fp16 value this launch writes is inf / nan, i.e. an activation left the
                            fp16 range (|x| > 65504).  NULL = no check; op_igemm fills it in itself while the range check is on
                            (ctrl_range_check / CTRL_CHECK_FINITE=1) */
} ctrl_igemm_desc;
int ctrl_op_igemm(const ctrl_igemm_desc* d, void* stream);
/* Test ABI.  The pinned form of the encoder plans: the 64 x 64 x 64 tile at every M, never split-K (row-major problems with
   Cin % 64 == 0 on the aligned vector epilogue; anything else is refused). */
int ctrl_op_igemm_pinned(const ctrl_igemm_desc* d, void* stream);
/* Test ABI.  n (1..4) problems as the plans launch the sibling adapter blocks of a pyramid level: ONE launch when the descriptors agree
   in everything but their addresses (and grouped launches are on, ctrl_group_launches), one launch each otherwise. */
int ctrl_op_igemm_group(const ctrl_igemm_desc* d, int n, void* stream);
/* Test ABI.  What ctrl_op_igemm would do with the descriptor's split-K scratch: the number of K splits (1 = none; depends on the
   descriptor's pointers and strides and on ctrl_igemm_set_wide), and the exact sizes of the scratch (bytes) and of the zeroed
   ticket words (int32 words; 0 = the in-launch reduction does not apply) for that many splits. */
int ctrl_igemm_splitk_factor(const ctrl_igemm_desc* d);
int64_t ctrl_igemm_splitk_ws_bytes(const ctrl_igemm_desc* d, int splits);
int64_t ctrl_igemm_splitk_ticket_words(const ctrl_igemm_desc* d, int splits);
/* Test ABI.  Which kernel form ctrl_op_igemm (pinned != 0: ctrl_op_igemm_pinned) would launch for the descriptor as one of group_n
   (1..4) same-form problems of a grouped launch, written to buf (cap bytes) as the launch would record it: the kernel symbol with
   its template arguments, then " splitkN" for a split problem and " in-launch" where that reduction is taken.  Depends on the
   descriptor, the policy table, ctrl_igemm_set_wide and ctrl_group_launches only: it launches nothing and needs no device. */
int ctrl_igemm_select(const ctrl_igemm_desc* d, int group_n, int pinned, char* buf, int cap);
/* Fused GEGLU feed-forward of a transformer block with dim 512 / hidden 2048 (csrc/ffn.hip; diffusers FeedForward(GEGLU) under
   BasicTransformerBlock / TemporalBasicTransformerBlock, model/adapter_spatial_temporal.py:108-130):
       out = epilogue( ((X W1h^T + b1h) * gelu_erf(X W1g^T + b1g)) W2^T )
   in ONE launch -- the [M][2048] hidden activation never reaches HBM.  X fp16 [M][ldx] (the LayerNorm output), W1 / b1 the GEGLU-
   interleaved pack of ff.net.0.proj (ctrl_op_pack_linear_w / ctrl_op_pack_vec with geglu = 1: [4096][512], [4096]), W2p the pack of
   ff.net.2 re-ordered along K by ctrl_op_ffn_pack_w2, `out` the descriptor of the OUTPUT GEMM ([M][512]: bias, res / ldres / res_f32,
   seg[0] row-major, out16 ...; its A / W / K fields are ignored).  ctrl_op_ffn_pack_w2: fp16 [512][2048] linear pack -> fp16 [512][2048].
   Of the output descriptor the kernel honours bias, res / ldres / res_f32, seg[0] (row-major, fp16 or fp32, all 512 columns), out16 / ld16,
   the AlphaBlender fold (blend_*) and nonfinite; every row stride must be a multiple of 8 elements and every one of those pointers
   16-byte aligned (the epilogue moves 16-byte pieces); rowvec, act, geglu, res_up = 2, a scale other than 1, scale2_from, out16_lo_off
   and a bf16 output are refused. */
typedef struct ctrl_ffn_desc {
    const void* X; int64_t ldx;
    const void* W1; const float* b1;
    const void* W2p;
    ctrl_igemm_desc out;
} ctrl_ffn_desc;
int ctrl_op_ffn(const ctrl_ffn_desc* d, void* stream);
/* Test ABI.  d[0..n), 1 <= n <= 4, equal M: the feed-forwards of sibling adapter blocks in ONE launch, the way the plans' collector
   launches them (member g owns workgroups [g * per, g * per + ceil(M / 128)), per = ceil(M / 128) rounded up to a multiple of 8;
   the rest exit at once); the result of every member is bit for bit what ctrl_op_ffn gives it alone. */
int ctrl_op_ffn_group(const ctrl_ffn_desc* d, int n, void* stream);
int ctrl_op_ffn_pack_w2(const void* w2_packed, void* out, int N, int K, void* stream);
/* Range safety of the fp16 activations (debug aid for real checkpoints: the synthetic N(0, 0.02^2) weights never leave the fp16 range).
   ctrl_range_check(1) -- or CTRL_CHECK_FINITE=1 in the environment -- makes every GEMM / convolution epilogue OR "this fp16 value is
   inf / nan" into a per-device flag word; ctrl_range_check(0) turns it off, ctrl_range_check(-1) only queries.  ctrl_range_status(reset)
   synchronises the current device and returns 1 when the flag was raised since the last reset (2 = the check is off).  The Python
   mirrors call it after every forward while the check is on and raise RuntimeError. */
int ctrl_range_check(int on);
int ctrl_range_status(int reset);
/* Walk order of the GEMM's output tiles over the 8 XCDs (csrc/tile_order.h; performance only, results are identical):
   "auto" (default; also CTRL_IGEMM_ORDER: grouped walk for row GEMMs whose weights exceed an XCD's L2 share), "legacy", or
   forced "m,G" / "n,G" (XCDs split the activation panels / the weight panels, weight panels walked in groups of G tiles).
   0 = accepted.
   ctrl_igemm_tile_of: the (tile_m, tile_n) workgroup `bid` of an ntm x ntn grid computes under (mode 0|1|2, group) --
   a diagnostic the host tests use to prove every order is a bijection. */
int ctrl_igemm_set_order(const char* spec);
/* Which problems run on the 8-phase wide-tile kernel (csrc/igemm.hip: igemm8_kernel, 256 x 256|320 x 64 tiles): 0 none (the round-3
   ring kernels), 1 wherever the grid fills the chip (default; also CTRL_IGEMM8=0|1|force), 2 every eligible problem whatever its
   size -- what the parity tests use to drive their small shapes through it.  -1 restores the default.  Performance only: both
   kernel families share one epilogue and the same accumulation order inside a k-tile; results may differ in the last fp32 bit
   between families (different k-tile depth).  0 = accepted. */
int ctrl_igemm_set_wide(int mode);
/* Grouped launches (csrc/ops.h: OpCollector): the sibling adapter blocks of one pyramid level -- equal shapes, independent
   (model/ctrl_adapter.py:181-191) -- are replayed in lock-step and every GEMM / GroupNorm / LayerNorm / attention of theirs leaves as
   ONE launch over 2-4 problems.  1 (default; also CTRL_GROUP) on: the GEMM dispatcher sizes its tile for the whole group (a 32^2 level
   reaches the wide tile), so results equal the one-by-one forward within the tile families' last-bit differences, like another batch
   size; 2 on with the tile every problem would get alone: bit-identical to the one-by-one forward; 0 off; -1 queries.  Returns the
   mode.  Every mode is bit-reproducible run to run. */
int ctrl_group_launches(int on);
/* Run-time policy table (csrc/policy.h): every CTRL_* environment variable the library understands is read ONCE, at the first query, into
   one table -- no dispatcher, plan or op calls getenv().  Test / experiment ABI: ctrl_policy_set(name, value) overrides an entry for the
   process (value NULL = unset; 0 = accepted, 1 = unknown name), ctrl_policy_get(name) returns the value in force (NULL = unset or unknown),
   ctrl_policy_count / ctrl_policy_name(i) list the names (a bench line can record what a run was taken with).  Not to be called
   concurrently with a forward. */
int ctrl_policy_set(const char* name, const char* value);
const char* ctrl_policy_get(const char* name);
int ctrl_policy_count(void);
const char* ctrl_policy_name(int i);
int ctrl_igemm_tile_of(int bid, int ntm, int ntn, int mode, int group, int* tile_m, int* tile_n);

typedef struct ctrl_attn_desc {
    const void* Q; int64_t ldq;      /* [B*Lq][ldq] fp16, head h at column h*D */
    const void* K; int64_t ldk;      /* [kvB*Lk][ldk] */
    const void* Vt; int32_t Lkpad; int32_t kvB;     /* [kvB][heads*D][Lkpad], Lkpad % 64 == 0; kvB = B, or 1 = K/V shared by all batches */
    void* O; int64_t ldo;            /* [B*Lq][ldo] */
    int32_t B, heads, D, Lq, Lk;
    float scale;
    int32_t k_prescaled;             /* K rows already hold k * scale * log2(e) (applied in fp32 by the producing GEMM's epilogue,
                                        before the one rounding to fp16): the kernel then folds the running maximum into the
                                        accumulator initialisation of the QK^T MFMA and exponentiates its output directly */
    int32_t pad0_;
} ctrl_attn_desc;
int ctrl_op_flash_attn(const ctrl_attn_desc* d, void* stream);
/* d[0..n), 1 <= n <= 4: the attentions of sibling adapter blocks.  Problems that agree in every shape, stride, scale and in the 16-byte
   phase of their pointers share ONE launch (workgroup b works on problem b / workgroups-per-problem; with CTRL_GROUP=0, or when
   the members disagree, n launches in order); the result of every member is bit for bit what ctrl_op_flash_attn gives it alone. */
int ctrl_op_flash_attn_group(const ctrl_attn_desc* d, int n, void* stream);
/* Instruction-selection variant of the head_dim-64 long-sequence kernel (csrc/attention_d64.hip): 0 = the round-2 kernel,
   > 0 = the round-3 family (what each number selects is listed in that file); performance only, every variant computes the
   same function.  -1 = back to the default (CTRL_ATTN_VARIANT or the best measured).  Used by tools/attn_bench.cpp. */
int ctrl_attn_set_variant(int v);
/* The attention kernels' workgroup -> (batch * heads + head, query tile) map, evaluated on the host (CPU tests: every (pair, tile) exactly once,
   whole pairs per XCD, the last partial round balanced over the eight XCDs -- csrc/ops.h attn_work_map).  Returns 1 and fills pair / qtile when
   workgroup `gbid` of a grid of 8 * ceil(pairs / 8) * qtiles has work, 0 when it exits at once. */
int ctrl_attn_work_map(int gbid, int qtiles, int pairs, int* pair, int* qtile);

typedef struct ctrl_tattn_desc {
    const void* Q; int64_t ld;       /* [(b*Fq+f)*HW + p][ld], head h at column h*64; unsharded: rows are q | k | v, 3*C wide */
    void* O; int64_t ldo;            /* [rows][C] */
    int32_t Bc, F, HW, heads;        /* clips, key frames per clip (<= 32), pixels, heads of 64 */
    float scale;
    int32_t Fq;                      /* query frames per clip held in Q / O (0 = F) */
    /* keys / values: NULL = the k | v columns of the Q rows.  Otherwise K|V rows [((r*Bc + b)*Fl + fl)*HW + p][ldkv]
       (k at column h*64, v at C + h*64) for key frame kf = r*Fl + fl: the all-gathered K|V of a clip whose frames are
       sharded over ranks, Fl frames per rank */
    const void* KV; int64_t ldkv;
    int32_t Fl;                      /* key frames per gathered shard (0 = F) */
    int32_t pad0_;
} ctrl_tattn_desc;
int ctrl_op_temporal_attn(const ctrl_tattn_desc* d, void* stream);

/* x_dtype: CTRL_F16 or CTRL_F32 (fp32 residual stream).  GroupNorm statistics are reduced in a fixed order (no
 * floating-point atomics): `stats` holds ctrl_op_gn_stats_floats(...) floats - [imgs][G][2] (sum, sumsq) results first,
 * then scratch - and must have been zeroed once; the kernel leaves its scratch tickets zero again. */
size_t ctrl_op_gn_stats_floats(int imgs, int rows_per_img, int C, int G);
int ctrl_op_gn_stats(const void* x, int x_dtype, float* stats, int imgs, int rows_per_img, int C, int G, void* stream);
int ctrl_op_gn_apply(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y,
                     int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream);
/* split-operand variant: y rows are [hi | lo] (row stride ldy, lo at column offset lo_off), hi + lo = the fp32 result to ~2^-22 */
int ctrl_op_gn_apply_split(const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta, void* y,
                           int64_t ldy, int lo_off, int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream);
/* GroupNorm(32) of a small map in ONE launch (statistics + apply by the same workgroup; qualifies when the 80-channel slice of one
 * image is at most 512 KB: ctrl_op_gn_fused_applies): ldy = row stride of y (0 = C), lo_off > 0 = split [hi | lo] result as above.
 * The plans use it only with CTRL_GN_FUSED=1: measured inside the step it is slower than the two launches it replaces. */
int ctrl_op_gn_fused_applies(int x_dtype, int rows_per_img, int C, int G);
int ctrl_op_gn_fused(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int64_t ldy, int lo_off,
                     int imgs, int rows_per_img, int C, int G, float eps, int silu, void* stream);
int ctrl_op_layernorm(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                      int M, int C, float eps, void* stream);
/* Test ABI of the norm kernels (tests/norm_forms.py): every argument of the op layer, and its grouped launches.
   ctrl_gn_desc: one GroupNorm problem.  ldx: elements between the rows of x (0 = C; larger: x is a column range of wider rows);
   ldy: row stride of y (0 = C); lo_off > 0: the row also carries lo = fp16(v - hi) at column lo_off; stat_rows: rows per image the sums in
   `stats` span (0 = rows_per_img; larger when they were added over row shards); y_img_rows / y_row0: image i of y starts at row
   i * y_img_rows + y_row0 (0 = dense).  The statistics pass reads x, x_dtype, stats, imgs, rows_per_img, C, G, ldx; the fused form
   (ctrl_op_gn_fused_applies) ignores stats, stat_rows, y_img_rows, y_row0 and ldx. */
typedef struct ctrl_gn_desc {
    const void* x; int32_t x_dtype; int32_t silu;
    float* stats; const float* gamma; const float* beta; void* y;
    int32_t imgs, rows_per_img, C, G;
    float eps; int32_t lo_off;
    int64_t ldx, ldy, stat_rows, y_img_rows, y_row0;
} ctrl_gn_desc;
/* d[0..n), 1 <= n <= 4: problems that agree in every shape argument share ONE launch (problem = blockIdx.z), others are launched one by
   one; every member's result is bit for bit what it gets alone */
int ctrl_op_gn_stats_group(const ctrl_gn_desc* d, int n, void* stream);
int ctrl_op_gn_apply_group(const ctrl_gn_desc* d, int n, void* stream);
int ctrl_op_gn_fused_group(const ctrl_gn_desc* d, int n, void* stream);
/* rows per workgroup and workgroups (chunks) per image of the statistics (pass 0) / apply (pass 1) launch for a shape, as the launchers
   compute them; launches nothing, needs no device.  0 = filled */
int ctrl_gn_launch_shape(int imgs, int rows_per_img, int C, int pass, int* rows_per_block, int* chunks);
/* one LayerNorm problem; addv (optional, fp32 [vmod][ldv]): xsum[m] = x[m] + addv[(m / rows_per_img) % vmod] is written (x's dtype, row
   stride ldx) and normalised */
typedef struct ctrl_ln_desc {
    const void* x; int32_t x_dtype; int32_t M;
    int64_t ldx;
    const float* addv; int64_t ldv; int32_t rows_per_img, vmod; void* xsum;
    const float* gamma; const float* beta; void* y; int64_t ldy;
    int32_t C; float eps;
} ctrl_ln_desc;
int ctrl_op_layernorm_group(const ctrl_ln_desc* d, int n, void* stream);
int ctrl_op_layernorm_add(const void* x, int x_dtype, int64_t ldx, const float* addv, int64_t ldv, int rows_per_img, int vmod, void* xsum,
                          const float* gamma, const float* beta, void* y, int64_t ldy, int M, int C, float eps, void* stream);
/* Test ABI of the small streaming kernels (tests/test_gpu_stream_forms.py).  add_rowvec_clip: rows (clip b, frame, pixel p) of x get
   v[(b * L + p) % B] added; upsample2x_nhwc: nearest x2 of an fp16 NHWC map; fill_zero_group: 1..4 zero fills of any alignment and size in
   one launch; linear_small_group: `count` independent ctrl_op_linear_small problems, 40 per launch; frameidx_sincos: ctrl_op_timestep_sincos
   with t[n] = n % F */
int ctrl_op_add_rowvec_clip(const void* x, int x_dtype, const float* v, int64_t ldv, void* y, int y_dtype, int B, int F, int L, int C,
                            void* stream);
int ctrl_op_upsample2x_nhwc(const void* x, void* y, int N, int H, int W, int C, void* stream);
int ctrl_op_fill_zero_group(void* const* p, const size_t* bytes, int n, void* stream);
typedef struct ctrl_small_lin {
    const float* x; int64_t ldx; const void* w; const float* b; float* out; int64_t ldo;
    int32_t M, N, K, in_silu, out_silu, pad0_;
} ctrl_small_lin;
int ctrl_op_linear_small_group(const ctrl_small_lin* p, int count, void* stream);
int ctrl_op_frameidx_sincos(float* out, int N, int F, int dim, void* stream);
int ctrl_op_nchw_to_nhwc(const void* x, int dtype, void* y, int N, int C, int HW, void* stream);
int ctrl_op_nhwc_to_nchw(const void* x, void* y, int dtype, int N, int C, int HW, float scale, void* stream);
int ctrl_avgpool_nchw(const void* x, void* y, int dtype, int NC, int Hin, int Win, int Hout, int Wout, void* stream);
int ctrl_op_timestep_sincos(const float* t, int t_count, float* out, int N, int dim, void* stream);
int ctrl_op_linear_small(const float* x, int64_t ldx, const void* w, const float* b, float* out, int64_t ldo,
                         int M, int N, int K, int in_silu, int out_silu, void* stream);
int ctrl_op_blend(const void* x_spatial, int xs_dtype, const void* x_temporal, int xt_dtype, const float* mix_factor,
                  void* y, int y_dtype, size_t n, void* stream);
int ctrl_op_add_rowvec(const void* x, int x_dtype, const float* v, int64_t ldv, void* y, int y_dtype, size_t M, int C,
                       int rows_per_img, int vmod, void* stream);
int ctrl_op_conv3x3_direct(const void* in, int in_dtype, int in_nchw, const float* w, const float* bias, void* out,
                           int N, int Cin, int Cout, int Hin, int Win, int stride, int silu, void* stream);
/* Test ABI.  The fp32 stem forms of the direct kernel, which write the residual stream of the backbone UNets (stride 1, pad 1, + bias,
 * no activation; w fp32 [9][Cin][Cout], out fp32 rows [N*H*W][Cout], Cout % 16 == 0, out 16-byte aligned):
 *   ctrl_op_conv3x3_direct_f32  in = NCHW [N][Cin][H][W] of in_dtype, Cin = 4 | 8
 *   ctrl_op_conv3x3_rows_f32    in = fp32 channels-last rows [N*H*W][8] (16-byte aligned), Cin = 8 */
int ctrl_op_conv3x3_direct_f32(const void* in, int in_dtype, const float* w, const float* bias, void* out, int N, int Cin, int Cout,
                               int H, int W, void* stream);
int ctrl_op_conv3x3_rows_f32(const void* in, const float* w, const float* bias, void* out, int N, int Cin, int Cout, int H, int W,
                             void* stream);
/* the same 3x3 convolution (pad 1, stride 1|2, + bias, optional SiLU) on the matrix cores for channels-last fp16 input with Cin, Cout in
 * {16, 32}: w fp16 [Cout][9][Cin] (ctrl_op_pack_conv_w with taps = 9) */
int ctrl_op_conv3x3_small_mfma(const void* x, const void* w, const float* bias, void* out, int N, int Cin, int Cout, int Hin, int Win,
                               int stride, int silu, void* stream);
/* Conditioning-image preparation feeding the path (model/ctrl_helper.py:268-296 prepare_images = per frame diffusers
 * VaeImageProcessor(do_convert_rgb, no normalisation).preprocess -> batch repeat -> CFG duplication), bit-exact with Pillow's
 * 8-bit Lanczos resampling: src uint8 RGB [F][Hin][Win][3]; per resampled axis the bounds int32 [out][2] and the 22-bit
 * fixed-point weights int32 [out][ks] of Pillow's precompute_coeffs (device; NULL when the axis keeps its size); tmp uint8
 * [F][Hin][W][3]; out [cfg][repeat*F][3][H][W] in out_dtype, out[g][r*F + f] = frame f / 255 */
int ctrl_prepare_images(const void* src_u8, int F, int Hin, int Win, const int32_t* hbounds, const int32_t* hk, int hks,
                        const int32_t* vbounds, const int32_t* vk, int vks, void* tmp_u8, void* out, int out_dtype,
                        int W, int H, int repeat, int cfg, void* stream);
/* Canny condition extraction (model/ctrl_helper.py:171-179: cv2.Canny(np.array(img), 100, 200), then the edge map three times along the
 * channel axis), bit for bit OpenCV's Canny with apertureSize 3 and the L1 magnitude, for N images of one size in one call.
 *   src_u8 uint8 [N][H][W][C], C = 1 | 3 (device; any byte alignment); low / high as cv2 takes them: swapped when low > high, then floored
 *   map    uint8 [N][H][W]: 0 no candidate, 1 weak, 2 strong (ctrl_op_canny_map writes it, ctrl_op_canny_hysteresis promotes every weak
 *          pixel 8-connected to a strong one, ctrl_op_canny_finish turns it into 0 / 255 as [N][H][W] (out_channels 1) or [N][H][W][3])
 *   ws     device scratch, 4-byte aligned: ctrl_canny_ws_bytes(N, H, W) bytes for ctrl_canny (a 256-byte flag block, then the map);
 *          ctrl_op_canny_hysteresis uses the flag block only
 *   *passes    hysteresis passes up to and including the first that promoted nothing; *readbacks  flag readbacks (each a stream
 *          synchronisation; CTRL_CANNY_BATCH passes are enqueued per readback)
 * The hysteresis loop reads a flag back between launches: ctrl_op_canny_hysteresis and ctrl_canny refuse a capturing stream.  Every entry
 * returns non-zero (ctrl_last_error) for a null pointer, C or out_channels outside {1, 3}, N, H or W < 1, and N*H*W*3 beyond 2^31 - 1 bytes
 * (ctrl_canny_ws_bytes returns 0 for such sizes).  ctrl_canny_launch_shape: the tile (pixels) one workgroup of the map and of the hysteresis
 * kernel owns -- where the tests put their edges. */
int ctrl_op_canny_map(const void* src_u8, int N, int H, int W, int C, double low, double high, void* map, void* stream);
int ctrl_op_canny_hysteresis(void* map, int N, int H, int W, void* ws, int64_t ws_bytes, int* passes, int* readbacks, void* stream);
int ctrl_op_canny_finish(const void* map, int N, int H, int W, int out_channels, void* out, void* stream);
int ctrl_canny(const void* src_u8, int N, int H, int W, int C, double low, double high, int out_channels, void* out, void* ws,
               int64_t ws_bytes, int* passes, int* readbacks, void* stream);
int64_t ctrl_canny_ws_bytes(int N, int H, int W);
int ctrl_canny_launch_shape(int H, int W, int* tile_h, int* tile_w);
/* load-time packers */
int ctrl_op_pack_conv_w(const void* w, int dtype, void* out, int Cout, int Cin, int taps, void* stream);
/* weights of a split-operand convolution: [Cout][taps][2*Cin], every tap's Cin weights twice (for the hi and the lo half) */
int ctrl_op_pack_conv_w_dup(const void* w, int dtype, void* out, int Cout, int Cin, int taps, void* stream);
int ctrl_op_pack_conv_w_direct(const void* w, int dtype, float* out, int Cout, int Cin, void* stream);
/* 3x3 conv weight [Cout][Cin][3][3] -> the phase pack fp16 [4][Cout][4][Cin] of ctrl_igemm_desc::mode 3: phase 2a + b, tap 2ty + tx =
   the sum of w[..][ky][kx] over ky in S(a, ty), kx in S(b, tx), S(0,0) = {0}, S(0,1) = {1,2}, S(1,0) = {0,1}, S(1,1) = {2}; summed
   in fp32 in (ky, kx) order, rounded to fp16 once */
int ctrl_op_pack_conv_w_phase(const void* w, int dtype, void* out, int Cout, int Cin, void* stream);
int ctrl_op_pack_linear_w(const void* w, int dtype, void* out, int N, int K, int geglu, void* stream);
int ctrl_op_pack_vec(const void* v, int dtype, float* out, int N, int geglu, void* stream);
/* Test ABI of the helper kernels (tests/helper_forms.py, tests/test_gpu_helper_forms.py).
   The GEMM-weight packers with the fp16 range flag the plans pass: ovf (device int32, may be NULL) is set to 1 when a value to store --
   judged in fp32, before the rounding -- lies outside [-65504, 65504] or is inf / nan; it is never cleared.
   nhwc_to_nchw_map: ctrl_op_nhwc_to_nchw with img_map (device int32 [N], may be NULL): source image n is written as image img_map[n].
   unet_conv_out: 3x3, pad 1, x fp16 channels-last [N][H][W][C] (16-byte aligned, C a multiple of 8 from 16), w fp32 [9][C][Cout]
   (ctrl_op_pack_conv_w_direct), Cout <= 4, + bias -> out in out_dtype; layout 0: [N][Cout][H][W], 1: [N / frames][Cout][frames][H][W]
   (image n = (b, f)), 2: channels-last rows [N*H*W][Cout].
   i2v_frames: [B][4][F][HW] of dtype -> fp32 [(b f)][4][HW].
   vae_conv_in: one image, NCHW pixels [3][H][W] of dtype, w fp32 [9][3][Cout], Cout % 16 == 0 -> fp32 rows [H*W][Cout] (16-byte aligned) */
int ctrl_op_pack_conv_w_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int taps, int32_t* ovf, void* stream);
int ctrl_op_pack_conv_w_dup_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int taps, int32_t* ovf, void* stream);
int ctrl_op_pack_conv_w_phase_ovf(const void* w, int dtype, void* out, int Cout, int Cin, int32_t* ovf, void* stream);
int ctrl_op_pack_linear_w_ovf(const void* w, int dtype, void* out, int N, int K, int geglu, int32_t* ovf, void* stream);
int ctrl_op_nhwc_to_nchw_map(const void* x, void* y, int dtype, int N, int C, int HW, float scale, const int32_t* img_map, void* stream);
int ctrl_op_unet_conv_out(const void* x, const float* w, const float* bias, void* out, int out_dtype, int N, int H, int W, int C, int Cout,
                          int layout, int frames, void* stream);
int ctrl_op_i2v_frames(const void* x, int dtype, float* y, int B, int F, int HW, void* stream);
int ctrl_op_vae_conv_in(const void* px, int dtype, const float* w, const float* b, float* out, int H, int W, int Cout, void* stream);

/* ---------------------------------------------------------------- plan level */
/* A named view of one state-dict tensor (reference layout, device memory). */
typedef struct ctrl_tensor_ref {
    const char* name;
    const void* data;
    int32_t dtype;
    int32_t ndim;
    int64_t shape[6];
} ctrl_tensor_ref;

/* ---- ControlNet (SD-1.5 architecture family; controlnet/controlnet.py:179-438) ---- */
typedef struct ctrl_controlnet_config {
    int32_t in_channels;               /* 4 */
    int32_t conditioning_channels;     /* 3 */
    int32_t block_out_channels[4];     /* 320,640,1280,1280 */
    int32_t down_block_has_attn[4];    /* 1,1,1,0  (CrossAttnDownBlock2D x3, DownBlock2D) */
    int32_t layers_per_block;          /* 2 */
    int32_t num_attention_heads;       /* 8 (the reference's `attention_head_dim` naming quirk, :221-227) */
    int32_t cross_attention_dim;       /* 768 */
    int32_t cond_embed_channels[4];    /* 16,32,96,256 */
    float norm_eps;                    /* 1e-5 */
} ctrl_controlnet_config;

typedef struct ctrl_controlnet ctrl_controlnet;   /* opaque */

/* parameter inventory: names/shapes are the reference's state-dict keys (single source of truth for the
 * Python mirror).  Returns the number of parameters; fills name/shape for index i. */
int ctrl_controlnet_param_count(const ctrl_controlnet_config* cfg);
int ctrl_controlnet_param_spec(const ctrl_controlnet_config* cfg, int i, char* name, int name_len,
                               int64_t shape[6], int* ndim);
/* builds a plan: packs the weights (fp16, MFMA-friendly layouts) into memory owned by the plan */
int ctrl_controlnet_create(const ctrl_controlnet_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors,
                           void* stream, ctrl_controlnet** out);
/* a second plan over the SAME packed weights (reference-counted) with its own workspace / streams / events: lets two forwards of one
   module be in flight at once (the mirror's batch lanes).  ctrl_controlnet_destroy frees it; the weights go with the last holder. */
int ctrl_controlnet_clone(ctrl_controlnet* h, ctrl_controlnet** out);
void ctrl_controlnet_destroy(ctrl_controlnet* h);

enum { CTRL_SKIP_CONV_IN = 1, CTRL_SKIP_TIME_EMB = 2, CTRL_GUESS_MODE = 4,
       /* step-invariant caching of the conditioning embedder (controlnet/controlnet.py:94-104): the condition image is the
        * same on every denoise step of a request.  KEEP = also store the embedder's last hidden map (256 ch at the latent
        * resolution) in plan-owned memory; REUSE = controlnet_cond is unchanged since the forward that stored it: start
        * from the stored map (only the final zero-initialised 3x3 conv runs).  Results are bit-identical either way. */
       CTRL_COND_KEEP = 8, CTRL_COND_REUSE = 16,
       /* everything on the launch stream, no auxiliary lane: for callers that already run this forward on a forked lane of their own
        * (MultiControlNetModel's per-net lanes) -- a fork inside a fork crashes hipGraph's end-of-capture on ROCm 7.2 */
       CTRL_NO_AUX_LANE = 32 };
/* sample [N][4][Hs][Ws], timesteps fp32 device [t_count] (1 or N), encoder_hidden_states [N][Lk][cross],
 * controlnet_cond [N][3][8*Hs][8*Ws]; outs[0..11] = down_block_res_samples, outs[12] = mid_block_res_sample,
 * all NCHW in out_dtype, already multiplied by conditioning_scale. */
int ctrl_controlnet_forward(ctrl_controlnet* h,
                            const void* sample, int sample_dtype, int N, int Hs, int Ws,
                            const float* timesteps, int t_count,
                            const void* encoder_hidden_states, int ehs_dtype, int Lk,
                            const void* controlnet_cond, int cond_dtype,
                            float conditioning_scale, int flags,
                            void* const* outs, int out_dtype, void* stream);

/* ---- Ctrl-Adapter (model/ctrl_adapter.py:17-116) ---- */
typedef struct ctrl_adapter_config {
    int32_t backbone_sdxl;             /* 1: up-sampling scale 2 (ctrl_adapter.py:61-66) */
    int32_t num_blocks;                /* layers per adapter block (configs use 1) */
    int32_t num_adapters_per_location; /* 1|2|3 */
    int32_t cross_attention_dim;       /* 2048 (sdxl) | 1024 (i2vgen-xl, svd) */
    int32_t add_spatial_resnet, add_temporal_resnet, add_spatial_transformer, add_temporal_transformer;
    int32_t loc_A, loc_B, loc_C, loc_D, loc_M;
} ctrl_adapter_config;

typedef struct ctrl_adapter ctrl_adapter;
int ctrl_adapter_param_count(const ctrl_adapter_config* cfg);
int ctrl_adapter_param_spec(const ctrl_adapter_config* cfg, int i, char* name, int name_len,
                            int64_t shape[6], int* ndim);
int ctrl_adapter_create(const ctrl_adapter_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors,
                        void* stream, ctrl_adapter** out);
void ctrl_adapter_destroy(ctrl_adapter* h);
/* ins[0..11] down_block_res_samples, ins[12] mid (may be NULL) : NCHW [N][C_i][H_i][W_i] in in_dtype, with
 * (H_0,W_0) = (H0,W0) and the SD-1.5 pyramid below it.  outs[i] NCHW in out_dtype at the adapted
 * resolution (x2 for sdxl); slots without an adapter are zero-filled (zeros_like, ctrl_adapter.py:193).
 * outs[12] may be NULL.  encoder_hidden_states [ehs_batch][Lk][cross], ehs_batch = 1 (broadcast) or N. */
int ctrl_adapter_forward(ctrl_adapter* h,
                         const void* const* ins, int in_dtype, int N, int H0, int W0, int num_frames,
                         const float* timesteps, int t_count,
                         const void* encoder_hidden_states, int ehs_dtype, int ehs_batch, int Lk,
                         void* const* outs, int out_dtype, void* stream);
/* The same forward with the pipelines' "sparse frames -> dense frames" scatter folded into the last epilogue of every
 * block (i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:1052-1071, svd/pipelines/
 * svd_controlnet_adapter_pipeline.py:719-741: torch.zeros + a python loop of per-frame copies): outs[i] hold N_out
 * frames, input frame j is written at frame frame_pos[j] (host array of N distinct positions < N_out), every other
 * frame is zero-filled.  The values are bit-identical to ctrl_adapter_forward's; only their location differs. */
int ctrl_adapter_forward_scatter(ctrl_adapter* h,
                                 const void* const* ins, int in_dtype, int N, int H0, int W0, int num_frames,
                                 const float* timesteps, int t_count,
                                 const void* encoder_hidden_states, int ehs_dtype, int ehs_batch, int Lk,
                                 void* const* outs, int out_dtype, const int32_t* frame_pos, int N_out, void* stream);

/* ---- Step-invariant text K/V cache: the to_k / to_v projections of encoder_hidden_states of every
 * cross-attention (Lk > 1) are kept in plan-owned buffers.  mode 1 (keep): the next forwards compute and store them (run
 * the first one eagerly, not under stream capture: it allocates); mode 2 (reuse): the projection GEMMs are skipped and
 * the stored K / V^T are read -- valid while encoder_hidden_states (values, batch, length) are unchanged, which the
 * caller guarantees; mode 0: off (default).  Results are bit-identical in all three modes. */
int ctrl_controlnet_text_cache(ctrl_controlnet* h, int mode);
int ctrl_adapter_text_cache(ctrl_adapter* h, int mode);

/* ---- Workspace hygiene.  A plan's workspace, text K/V buffers and conditioning cache grow by RETIRING the outgrown block
 * (never freeing it inside a forward: queued launches and captured hipGraphs keep valid addresses), so a server that sees
 * ever larger shapes keeps the sum of the earlier sizes.  ctrl_*_trim synchronises the device and frees the retired blocks;
 * call it when no captured graph that was recorded before the last growth will be replayed again.  A plan has no lock: trim
 * must not run concurrently with a forward of the same plan, and it is refused (non-zero) while a stream capture of that plan's
 * forward is still open (its device synchronisation would invalidate the capture). */
/* Which precision selection plan creation took for this checkpoint (a short key=value line): split-operand levels, whether outlier
   normalisation scales (max|gamma| / median|gamma| above the gate) switched it to the conservative selection, fp32 token-stream blocks of
   the adapter.  The Python mirrors expose it as `module.selection` and warn once when a conservative selection was taken. */
int ctrl_controlnet_selection(ctrl_controlnet* h, char* buf, int len);
int ctrl_adapter_selection(ctrl_adapter* h, char* buf, int len);
int ctrl_controlnet_trim(ctrl_controlnet* h);
int ctrl_adapter_trim(ctrl_adapter* h);

/* ---- One clip split across GPUs by frames (BASELINE.json config 4 with clips < GPUs).
 * Every rank holds Fl = F / world consecutive frames of every clip: `N` = clips * Fl LOCAL frames (frame-major, rank r
 * owns frames [r*Fl, (r+1)*Fl) of each clip), num_frames = Fl.  All ops of the adapter are per frame except three, and
 * each of those does exactly one exchange through the caller-supplied transport (stream-ordered on `stream`; byte
 * offsets into the exchange workspace `ws`, which the caller registered with its transport):
 *   temporal transformer (model/adapter_spatial_temporal.py:280) all_to_all: frame shards <-> pixel shards around the block
 *                       (everything inside it is per pixel), or -- when the transport has no all_to_all or the
 *                       pixels do not divide by the ranks -- all_gather of the K|V rows over the frame axis
 *   Conv3d (3,1,1)      (TemporalResnetBlock, :226)              halo_exchange of the first / last local frame
 *   temporal GroupNorm  (TemporalResnetBlock, :226)              all_reduce_sum_f32 of the (clip, group) sums
 * The transports used are torch.distributed over RCCL (ctrl-adapter_amd/clip_parallel.py); any transport with these
 * semantics works.  Callbacks return 0 on success.  If `ws_bytes` is too small the call fails with return code 2 and
 * `ws_needed` holds the size to retry with.  Runs on the caller's stream only (no stream lanes).
 * Results: the all_gather form is BIT-identical to the unsharded forward; the all_to_all form is tolerance-equal (<= 3.4e-4
 * rel-inf observed, 1e-3 asserted) -- its way back carries the temporal branch as fp16 and the AlphaBlender runs after it,
 * where the unsharded path blends in the fp32 epilogue of the block's last GEMM.  When the pixels of a frame do not divide by
 * the ranks the all_to_all form is dropped for that block (logged once on stderr). */
typedef struct ctrl_clip_comm {
    int32_t rank, world;
    void* ws; int64_t ws_bytes;
    /* recv[r*bytes .. (r+1)*bytes) = rank r's send[0 .. bytes) */
    int (*all_gather)(void* user, int64_t send_off, int64_t recv_off, int64_t bytes_per_rank, void* stream);
    /* count floats at off, summed over ranks in place */
    int (*all_reduce_sum_f32)(void* user, int64_t off, int64_t count, void* stream);
    /* send_prev -> rank-1's recv_next, send_next -> rank+1's recv_prev (edge ranks have no such neighbour: nothing is
       sent and the corresponding recv area is left untouched) */
    int (*halo_exchange)(void* user, int64_t send_prev_off, int64_t send_next_off, int64_t recv_prev_off, int64_t recv_next_off,
                         int64_t bytes, void* stream);
    void* user;
    int64_t ws_needed;
    /* optional (NULL: the K|V all_gather form is used): recv[r*bytes .. (r+1)*bytes) = rank r's send[me*bytes .. (me+1)*bytes),
       i.e. block r of my send area goes to rank r.  Swaps frame shards for pixel shards around the temporal transformer:
       2 + 1 KB per token and direction instead of the 2*C*2 B x world a rank RECEIVES per token in the all_gather form
        */
    int (*all_to_all)(void* user, int64_t send_off, int64_t recv_off, int64_t bytes_per_rank, void* stream);
    /* optional: further transports (own communicator, own workspace `ws`) for the adapter's stream lanes.  The blocks of the four
       pyramid levels are independent, and on whole clips they run on four HIP streams; with ONE transport the sharded forward stays
       on the caller's stream (the exchanges of one communicator must be issued and executed in one order on every rank), which
       alone costs ~17 % at world 1.  A chain of L transports lets lane l issue its exchanges on transport l: every rank walks the
       same program, so every communicator still sees its calls in one order, and the all-to-all of a 128^2 block runs under the
       other lanes' compute.  rank / world must agree along the chain; ws_needed is reported on the head for all of them. */
    struct ctrl_clip_comm* next_lane;
} ctrl_clip_comm;
int ctrl_adapter_forward_clip_sharded(ctrl_adapter* h,
                                      const void* const* ins, int in_dtype, int N, int H0, int W0, int num_frames,
                                      const float* timesteps, int t_count,
                                      const void* encoder_hidden_states, int ehs_dtype, int ehs_batch, int Lk,
                                      void* const* outs, int out_dtype, const int32_t* frame_pos, int N_out,
                                      ctrl_clip_comm* comm, void* stream);

/* ---- The production transport, native: RCCL over xGMI, enqueued on the forward's stream from C++ (csrc/clip_rccl.cpp).  No host
 * callback into Python sits between launches, so ctrl_adapter_forward_clip_sharded is hipGraph-capturable with it (under capture the
 * forward uses the head of a next_lane chain only: RCCL refuses several communicators on forked streams inside one capture).  RCCL is
 * resolved at run time (dlopen; the copy already loaded into the process wins).  Rank 0 of the clip's group draws a unique id, the
 * caller ships its 128 bytes to the other ranks (any channel), every rank creates the communicator (collective), binds its
 * exchange workspace and passes the filled ctrl_clip_comm to the sharded forward. */
typedef struct ctrl_rccl_comm ctrl_rccl_comm;
int ctrl_rccl_unique_id(void* out128);
int ctrl_rccl_comm_create(const void* id128, int rank, int world, ctrl_rccl_comm** out);
void ctrl_rccl_comm_destroy(ctrl_rccl_comm* c);
int ctrl_rccl_comm_bind(ctrl_rccl_comm* c, void* ws, int64_t ws_bytes, int use_all_to_all, ctrl_clip_comm* cs);
int64_t ctrl_rccl_comm_bytes_sent(const ctrl_rccl_comm* c);

/* ---- Fused step: ctrl_controlnet_forward + ctrl_adapter_forward[_scatter] of one denoise step as one call (the two
 * back-to-back calls of the pipelines, sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1323,1338 and
 * svd/...:684,709, i2vgen_xl/...:957,1042).  Same arguments as the two calls (the ControlNet outputs cn_outs[13] are
 * the adapter inputs; use_mid = pass cn_outs[12] as mid_block_res_sample; frame_pos may be NULL = no scatter); same
 * results bit for bit; the ControlNet runs on a plan-owned stream and every adapter block starts as soon as ITS input
 * is ready.  CTRL_STEP_OVERLAP=0 runs the two halves back to back. */
int ctrl_step_forward(ctrl_controlnet* cn, ctrl_adapter* ad,
                      const void* sample, int sample_dtype, int N, int Hs, int Ws,
                      const float* cn_timesteps, int cn_t_count,
                      const void* cn_encoder_hidden_states, int cn_ehs_dtype, int cn_Lk,
                      const void* controlnet_cond, int cond_dtype, float conditioning_scale, int flags,
                      void* const* cn_outs, int cn_out_dtype,
                      int num_frames, const float* ad_timesteps, int ad_t_count,
                      const void* ad_encoder_hidden_states, int ad_ehs_dtype, int ad_ehs_batch, int ad_Lk,
                      int use_mid, void* const* outs, int out_dtype, const int32_t* frame_pos, int N_out, void* stream);

/* ---- CLIP text encoder (transformers CLIPTextModel, the SD-1.5 text_encoder; model/ctrl_helper.py:34-41,300-457) ----
 * Pre-LN transformer: x = tok_emb[ids] + pos_emb[:L]; per layer x += out_proj(causal_attn(qkv(LN1(x)))), x += fc2(quick_gelu(fc1(LN2(x))));
 * last_hidden_state = final_layer_norm(x); pooled = last_hidden_state[argmax(ids)] when eos_token_id == 2 (the legacy rule of
 * SD-1.5's config), else at the first position of eos_token_id.  Residual stream fp32, GEMM operands fp16, head_dim 64, L <= 77
 * (<= 128). */
typedef struct ctrl_text_encoder_config {
    int32_t vocab_size;                /* 49408 */
    int32_t hidden_size;               /* 768 (<= 1024, multiple of 64) */
    int32_t intermediate_size;         /* 3072 (multiple of 64) */
    int32_t num_hidden_layers;         /* 12 */
    int32_t num_attention_heads;       /* 12 (hidden_size / heads must be 64) */
    int32_t max_position_embeddings;   /* 77 (<= 128) */
    int32_t eos_token_id;              /* 2 = the argmax rule */
    float layer_norm_eps;              /* 1e-5 */
} ctrl_text_encoder_config;
typedef struct ctrl_text_encoder ctrl_text_encoder;   /* opaque */
/* weights: the state-dict tensors under their transformers 4.x keys (text_model.embeddings.token_embedding.weight, ...,
 * text_model.encoder.layers.{i}.self_attn.q_proj.weight, ..., text_model.final_layer_norm.bias), any dtype, device memory;
 * packed into plan-owned memory (GEMM weights fp16, the embedding tables / norms / biases fp32) -- synchronises `stream` once */
int ctrl_text_encoder_create(const ctrl_text_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                             ctrl_text_encoder** out);
void ctrl_text_encoder_destroy(ctrl_text_encoder* h);
/* input_ids int64 device [N][L] (1 <= L <= max_position_embeddings); outputs in out_dtype (NULL = not written):
 * last_hidden [N][L][hidden], pooled [N][hidden], hidden_states [num_hidden_layers + 1][N][L][hidden] (the embedding output and the
 * stream after every layer, before the final LayerNorm: transformers' output_hidden_states).  Never synchronises; capturable.
 * Every prompt is computed by the same instruction sequence whatever N: its rows are bit-identical alone or inside a batch.
 * An id outside [0, vocab_size) is clamped and raises the plan's flag word (ctrl_text_encoder_id_status). */
int ctrl_text_encoder_forward(ctrl_text_encoder* h, const int64_t* input_ids, int N, int L, void* last_hidden, void* pooled,
                              void* hidden_states, int out_dtype, void* stream);
/* 1 when a forward since the last reset met an id outside the vocabulary; reset = 1 clears the flag.  Synchronises the device. */
int ctrl_text_encoder_id_status(ctrl_text_encoder* h, int reset);
/* op level (csrc/text.hip).  embed: x fp32 [N*L][C] = tok[clamp(ids)] + pos[l], y fp16 = LayerNorm(x; gamma, beta); tok / pos fp32;
 * bad (device, optional) set to 1 by an id outside [0, V).  attn: causal softmax(q k^T * scale) v per (prompt, head) over L <= 128
 * tokens, head_dim 64, qkv fp16 [N*L][ld] (q of head h at column h*64, k at heads*64 + h*64, v at 2*heads*64 + h*64), out fp16
 * [N*L][ldo].  final_ln: y [rows][C] (y_dtype) = LayerNorm(x [rows][C], x_dtype); with ids (int64 [rows / L][L]) and pooled, the
 * prompt's pooled row (rule of eos_token_id above) goes to pooled [rows / L][C] as well. */
int ctrl_op_text_embed(const int64_t* ids, const float* tok, const float* pos, int V, int N, int L, int C, float* x,
                       const float* gamma, const float* beta, float eps, void* y, int32_t* bad, void* stream);
int ctrl_op_text_attn(const void* qkv, int64_t ld, void* out, int64_t ldo, int N, int L, int heads, float scale, void* stream);
int ctrl_op_text_final_ln(const void* x, int x_dtype, int rows, int C, const float* gamma, const float* beta, float eps,
                          void* y, int y_dtype, const int64_t* ids, int L, int eos_token_id, void* pooled, void* stream);
/* The embed and final_ln ops accept C <= 1024, or multiples of 64 up to 2048 (wider instantiations; the C <= 1024 kernels are those
 * of the SD-1.5 encoder). */

/* ---- Text towers beyond SD-1.5 (transformers CLIPTextModelWithProjection: SDXL's OpenCLIP ViT-bigG text_encoder_2, hidden 1280,
 * exact gelu, a bias-free text_projection) ----
 * ctrl_text_encoder_create_ext takes the config above plus this extension; hidden_size may be a multiple of 64 up to 2048.  With
 * projection_dim > 0 the weights include text_projection.weight [projection_dim][hidden] and text_embeds[n] = pooled_fp32[n] .
 * W_proj^T is computed in fp32 from the fp32 final-LayerNorm row of prompt n (not from the rounded pooled output), per prompt.
 * gemm_form 0: every linear on the pinned 64 x 64 x 64 implicit GEMM (what ctrl_text_encoder_create uses; exact gelu then runs as a
 * separate fp32 pass after the GEMM); 1: the few-row split-K GEMM of csrc/text_gemm.hip (weights streamed once over all XCDs, split
 * and reduction order functions of (N, K) only).  Both are batch-invariant. */
typedef struct ctrl_text_encoder_ext {
    int32_t hidden_act;        /* 0 quick_gelu, 1 gelu (erf) */
    int32_t projection_dim;    /* 0 = none; else text_projection.weight [projection_dim][hidden] */
    int32_t gemm_form;         /* 0 the pinned form, 1 the few-row GEMM */
    int32_t reserved;          /* 0 */
} ctrl_text_encoder_ext;
int ctrl_text_encoder_create_ext(const ctrl_text_encoder_config* cfg, const ctrl_text_encoder_ext* ext, const ctrl_tensor_ref* tensors,
                                 int n_tensors, void* stream, ctrl_text_encoder** out);
/* ctrl_text_encoder_forward plus text_embeds [N][projection_dim] (out_dtype; needs a projection) and a choice of hidden states:
 * hidden_index -1 writes all num_hidden_layers + 1 states to hidden_states as ctrl_text_encoder_forward does; k in
 * [0, num_hidden_layers] writes only state k, as [N][L][hidden].  When last_hidden, pooled and text_embeds are all NULL the forward
 * stops after layer k; the state it writes is bit-identical to a full forward's.  Works on plans of ctrl_text_encoder_create as well.
 * Never synchronises; capturable once a forward of the same or a larger batch has run eagerly (the workspace does not grow under
 * capture). */
int ctrl_text_encoder_forward_ext(ctrl_text_encoder* h, const int64_t* input_ids, int N, int L, void* last_hidden, void* pooled,
                                  void* text_embeds, void* hidden_states, int hidden_index, int out_dtype, void* stream);
/* op level (csrc/text_gemm.hip): y [M][N] (y_dtype) = act(x [M][K] W^T + bias) (+ res), x / W fp16 row-major, bias fp32 [N] (NULL =
 * none), res fp32 [M][N] (NULL = none); act 0 none, 2 quick_gelu, 3 exact gelu; N % 16 == 0, K % 32 == 0, 16-byte aligned pointers.
 * ws: device scratch of ctrl_text_gemm_ws_bytes(M, N, K) bytes.  Row m of y depends on row m of x alone, bit for bit. */
int64_t ctrl_text_gemm_ws_bytes(int M, int N, int K);
int ctrl_op_text_gemm(const void* x, const void* W, const float* bias, int M, int N, int K, int act, const float* res, void* y,
                      int y_dtype, void* ws, int64_t ws_bytes, void* stream);
/* test ABI of the two towers' remaining kernels (tests/tower_forms.py, tests/test_gpu_tower_forms.py): what a plan alone reaches.
 * text_gemm_finish: y [M][ldy] (y_dtype) = act(sum over ws [splits][M][N] fp32 in split order + bias) (+ res fp32 [M][ldres]); N % 4 == 0.
 * text_proj: out [N][P] (out_dtype) = pooled32 [N][C] . Wp [P][C]^T, fp32.  text_store: y [n] (y_dtype) = x [n] fp32.
 * vision_vt: vt fp16 [N][C][Lkpad] = v fp16 [N*L][ld] transposed per image, columns L..Lkpad-1 zero; C % 32 == 0, Lkpad % 32 == 0.
 * text_final_ln_ext: ctrl_op_text_final_ln plus pooled32 [rows / L][C], the pooled row in fp32 (either pooled may be NULL). */
int ctrl_op_text_gemm_finish(const float* ws, int splits, int M, int N, const float* bias, int act, const float* res, int64_t ldres, void* y,
                             int y_dtype, int64_t ldy, void* stream);
int ctrl_op_text_proj(const float* pooled32, const float* Wp, int N, int C, int P, void* out, int out_dtype, void* stream);
int ctrl_op_text_store(const float* x, void* y, int y_dtype, int64_t n, void* stream);
int ctrl_op_vision_vt(const void* v, int64_t ld, void* vt, int N, int L, int C, int Lkpad, void* stream);
int ctrl_op_text_final_ln_ext(const void* x, int x_dtype, int rows, int C, const float* gamma, const float* beta, float eps,
                              void* y, int y_dtype, const int64_t* ids, int L, int eos_token_id, void* pooled, float* pooled32, void* stream);

/* ---- CLIP vision tower (transformers CLIPVisionModelWithProjection: the image_encoder of SVD and I2VGen-XL, CLIP ViT-H/14;
 * svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212, i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:366-396) ----
 * emb = [class_embedding ; patch_conv(pixels)] + position_embedding; x = pre_layrnorm(emb); pre-LN layers as in the text tower but
 * non-causal (flash attention, head_dim 40 / 64 / 80 / 160); last_hidden_state = x (no final LayerNorm); pooled = post_layernorm(x[:, 0]);
 * image_embeds = pooled_fp32 . visual_projection^T (fp32, no bias).  Residual stream fp32, GEMM operands fp16.  hidden_size a multiple
 * of 64 up to 2048, image_size % patch_size == 0, (image_size / patch_size)^2 + 1 <= 577 tokens. */
enum { CTRL_U8_NHWC = 3 };           /* pixel dtype: uint8 [N][H][W][3] (PIL's layout), read as x / 255 */
typedef struct ctrl_vision_encoder_config {
    int32_t image_size;                /* 224 */
    int32_t patch_size;                /* 14 */
    int32_t hidden_size;               /* 1280 */
    int32_t intermediate_size;         /* 5120 */
    int32_t num_hidden_layers;         /* 32 */
    int32_t num_attention_heads;       /* 16 */
    int32_t projection_dim;            /* 1024 */
    int32_t hidden_act;                /* 0 quick_gelu, 1 gelu (erf) */
    float layer_norm_eps;              /* 1e-5 */
    int32_t gemm_form;                 /* 0 the pinned implicit GEMM, 1 the few-row split-K GEMM (csrc/text_gemm.hip) */
} ctrl_vision_encoder_config;
typedef struct ctrl_vision_encoder ctrl_vision_encoder;   /* opaque */
/* parameter inventory under transformers' keys (vision_model.embeddings.class_embedding, ..., visual_projection.weight) */
int ctrl_vision_encoder_param_count(const ctrl_vision_encoder_config* cfg);
int ctrl_vision_encoder_param_spec(const ctrl_vision_encoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_vision_encoder_create(const ctrl_vision_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                               ctrl_vision_encoder** out);
void ctrl_vision_encoder_destroy(ctrl_vision_encoder* h);
/* pixels [N][3][S][S] (pixel_dtype CTRL_F32 / F16 / BF16) or [N][S][S][3] (CTRL_U8_NHWC), S = image_size, device memory.
 * mean_std (host, mean[3] then std[3]; NULL = the pixels are already normalised): (x - mean_c) / std_c in fp32 before the one rounding
 * to fp16.  Outputs in out_dtype (NULL = not written): last_hidden [N][L][hidden], pooled [N][hidden], image_embeds [N][projection_dim],
 * hidden_states as in ctrl_text_encoder_forward_ext (hidden_index -1: all num_hidden_layers + 1 states [layers + 1][N][L][hidden], k:
 * state k alone [N][L][hidden]; with no other output the layers after k are not run).  Every image is computed by the same instruction
 * sequence whatever N (both gemm forms).  Never synchronises; capturable once a forward of the same or a larger batch ran eagerly. */
int ctrl_vision_encoder_forward(ctrl_vision_encoder* h, const void* pixels, int pixel_dtype, int N, const float* mean_std,
                                void* last_hidden, void* pooled, void* image_embeds, void* hidden_states, int hidden_index,
                                int out_dtype, void* stream);
/* op level (csrc/vision.hip).  patchify: pixels as above -> im2col rows out fp16 [N * (S/p)^2][Kpad] (column c*p*p + ky*p + kx, zero from
 * 3*p*p on; Kpad a multiple of 64), optionally normalised.  embed: x fp32 [N*L][C] = pre_layrnorm([cls ; patch [N*(L-1)][C]] + pos [L][C]),
 * y fp16 = LayerNorm(x; g1, b1).  cls_ln: post-LayerNorm of row 0 of every image of x fp32 [N][L][C] into pooled (out_dtype) and
 * pooled32 (fp32), either may be NULL.  resize_aa: SVD's _resize_with_antialiasing on x * 2 - 1 (Gaussian blur with reflect padding,
 * bicubic align_corners), then (x + 1) / 2 and the optional normalisation -> out [N][3][OH][OW] in out_dtype; src fp32 / fp16 / bf16
 * NCHW in [0, 1] or uint8 NHWC. */
int ctrl_op_vision_patchify(const void* pixels, int pixel_dtype, int N, int image_size, int patch_size, const float* mean_std, void* out,
                            int Kpad, void* stream);
int ctrl_op_vision_embed(const float* patch_out, const float* class_embedding, const float* pos, int N, int L, int C, const float* pre_g,
                         const float* pre_b, const float* ln1_g, const float* ln1_b, float eps, float* x, void* y, void* stream);
int ctrl_op_vision_cls_ln(const float* x, int N, int L, int C, const float* gamma, const float* beta, float eps, void* pooled,
                          int out_dtype, float* pooled32, void* stream);
int ctrl_op_clip_resize_aa(const void* src, int src_dtype, int N, int H, int W, int OH, int OW, const float* mean_std, void* out,
                           int out_dtype, void* stream);

/* ---- KL-VAE encoder (diffusers AutoencoderKL / AutoencoderKLTemporalDecoder: Encoder + quant_conv + DiagonalGaussianDistribution;
 * the image latents of the SVD pipeline's _encode_vae_image and I2VGen-XL's prepare_image_latents) ---- */
typedef struct ctrl_vae_encoder_config {
    int32_t num_levels;              /* len(block_out_channels), 1..4 */
    int32_t block_out_channels[4];   /* multiples of 32, <= 2048 */
    int32_t layers_per_block;
    int32_t latent_channels;         /* 1..8 */
    int32_t norm_num_groups;         /* 32 */
    float norm_eps;                  /* 1e-6 */
} ctrl_vae_encoder_config;
typedef struct ctrl_vae_encoder ctrl_vae_encoder;   /* opaque */
/* parameters: diffusers' keys (encoder.conv_in.*, encoder.down_blocks.{i}.resnets.{j}.*, ..., quant_conv.*) */
int ctrl_vae_encoder_param_count(const ctrl_vae_encoder_config* cfg);
int ctrl_vae_encoder_param_spec(const ctrl_vae_encoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_vae_encoder_create(const ctrl_vae_encoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                            ctrl_vae_encoder** out);
void ctrl_vae_encoder_destroy(ctrl_vae_encoder* h);
/* output kinds of the forward and of ctrl_op_vae_posterior; the latent grid is h x w = H / 2^(num_levels-1) x W / 2^(num_levels-1) */
enum { CTRL_VAE_MODE = 0,       /* out [N][lat][h][w] = mean * scale */
       CTRL_VAE_SAMPLE = 1,     /* out [N][lat][h][w] = (mean + std * eps) * scale, eps [N][lat][h][w] in eps_dtype */
       CTRL_VAE_MOMENTS = 2 };  /* out [N][4*lat][h][w] = mean | logvar | std | var (logvar clamped to [-30, 20]; scale ignored) */
/* pixels [N][3][H][W] (CTRL_F32 / F16 / BF16) in device memory, H and W multiples of 2^(num_levels-1) and of 8.  An image's result
   is bit-identical whatever batch it is encoded in.  The first forward of a larger shape allocates the workspace (not under stream
   capture); every later one is capturable. */
int ctrl_vae_encoder_forward(ctrl_vae_encoder* h, const void* pixels, int pixel_dtype, int N, int H, int W, const void* eps,
                             int eps_dtype, float scale, int kind, void* out, int out_dtype, void* stream);
/* op level (csrc/vae.hip).  row_softmax: P[r][c] (fp16, row stride ldp) = softmax_c(S[r][c]) over c < L in fp32 (S row stride lds),
   P[r][c] = 0 for L <= c < Lpad.  posterior: x fp32 NHWC rows [N*h*w][ldx] (x_nchw = 0: the conv_out result) or NCHW planes
   [N][ldx][h][w] (x_nchw = 1: a MOMENTS output), first 2*lat channels read; wq fp32 [2*lat][2*lat] / bq [2*lat] = quant_conv (NULL: none);
   then as the forward's kinds above. */
int ctrl_op_vae_row_softmax(const float* S, int64_t lds, void* P, int64_t ldp, int rows, int L, int Lpad, void* stream);
int ctrl_op_vae_posterior(const float* x, int64_t ldx, int x_nchw, const float* wq, const float* bq, int N, int lat, int h, int w,
                          const void* eps, int eps_dtype, float scale, int kind, void* out, int out_dtype, void* stream);

/* ---- KL-VAE decoder (diffusers AutoencoderKL.decode: post_quant_conv + Decoder; the image decode of the SDXL pipeline and the frame
 * decode of I2VGen-XL's decode_latents) ---- */
typedef struct ctrl_vae_decoder_config {
    int32_t num_levels;              /* len(block_out_channels), 1..4 */
    int32_t block_out_channels[4];   /* as in the VAE's config (the decoder walks them reversed); multiples of 32, <= 2048 */
    int32_t layers_per_block;        /* every up block holds layers_per_block + 1 ResNets */
    int32_t latent_channels;         /* 1..8 */
    int32_t norm_num_groups;         /* 32 */
    float norm_eps;                  /* 1e-6 */
    int32_t out_channels;            /* 1..4 (3: RGB) */
} ctrl_vae_decoder_config;
typedef struct ctrl_vae_decoder ctrl_vae_decoder;   /* opaque */
/* parameters: diffusers' keys (post_quant_conv.*, decoder.conv_in.*, decoder.mid_block.*, decoder.up_blocks.{i}.resnets.{j}.*,
   decoder.up_blocks.{i}.upsamplers.0.conv.*, decoder.conv_norm_out.*, decoder.conv_out.*) */
int ctrl_vae_decoder_param_count(const ctrl_vae_decoder_config* cfg);
int ctrl_vae_decoder_param_spec(const ctrl_vae_decoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_vae_decoder_create(const ctrl_vae_decoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                            ctrl_vae_decoder** out);
void ctrl_vae_decoder_destroy(ctrl_vae_decoder* h);
/* epilogues of the forward and of ctrl_op_vae_dec_tail; x = conv_out's fp32 result, rounded to out_dtype first (what .sample holds);
   the image is H x W = h * 2^(num_levels-1) x w * 2^(num_levels-1) */
enum { CTRL_VAE_DEC_SAMPLE = 0,   /* out [N][out_channels][H][W] in out_dtype = x: decode(z).sample */
       CTRL_VAE_DEC_UNIT = 1,     /* out [N][out_channels][H][W] fp32 = clamp(x / 2 + 0.5, 0, 1): VaeImageProcessor.postprocess("pt") */
       CTRL_VAE_DEC_U8 = 2 };     /* out [N][H][W][out_channels] uint8 = rint(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even: numpy_to_pil */
/* latents [N][latent_channels][h][w] (CTRL_F32 / F16 / BF16) in device memory, multiplied by `scale` (1 / scaling_factor) on load.  An
   image's pixels are bit-identical whatever batch it is decoded in.  The first forward of a larger shape allocates the workspace (not
   under stream capture); every later one is capturable. */
int ctrl_vae_decoder_forward(ctrl_vae_decoder* h, const void* latents, int latent_dtype, int N, int lat_h, int lat_w, float scale, int kind,
                             void* out, int out_dtype, void* stream);
/* the same on latents that are not one dense block: image n starts image_stride elements after image n - 1 and its dense [h][w] channel
   planes lie channel_stride (>= h * w) elements apart.  The F frames of clip b of [B][C][F][h][w] latents (I2VGen-XL's decode_latents)
   are N = F images with image_stride = h * w and channel_stride = F * h * w: no permuted copy of the latents is needed. */
int ctrl_vae_decoder_forward_strided(ctrl_vae_decoder* h, const void* latents, int latent_dtype, int N, int lat_h, int lat_w,
                                     int64_t image_stride, int64_t channel_stride, float scale, int kind, void* out, int out_dtype,
                                     void* stream);
/* op level (csrc/vae.hip), one image each.  dec_head: z NCHW [lat][h][w] (z_dtype, ch_stride >= h * w elements between its channel
   planes) * scale -> post_quant_conv (wpq fp32 [lat][lat],
   bpq [lat]) -> conv_in 3x3 (w_in fp32 [9][lat][Cout] as ctrl_op_pack_conv_w_direct packs it, b_in [Cout]; Cout % 16 == 0), all fp32
   -> out fp32 NHWC [h*w][Cout].  dec_tail: x fp32 NHWC [H*W][C] -> GroupNorm(32) from `stats` (ctrl_op_gn_stats of x: sum | sum of
   squares per group) with gamma / beta, SiLU, conv_out 3x3 (w_out fp32 [9][C][Cout], b_out [Cout], Cout <= 4) in fp32 -> the epilogue
   `kind` above. */
int ctrl_op_vae_dec_head(const void* z, int z_dtype, float scale, const float* wpq, const float* bpq, const float* w_in, const float* b_in,
                         float* out, int lat, int h, int w, int64_t ch_stride, int Cout, void* stream);
int ctrl_op_vae_dec_tail(const float* x, const float* stats, const float* gamma, const float* beta, float eps, const float* w_out,
                         const float* b_out, int H, int W, int C, int Cout, int kind, void* out, int out_dtype, void* stream);

/* ---- Temporal KL-VAE decoder (diffusers AutoencoderKLTemporalDecoder.decode: the TemporalDecoder behind SVD's decode_latents).  The
 * config is the KL-VAE decoder's; there is no post_quant_conv. ---- */
typedef struct ctrl_vae_tdecoder ctrl_vae_tdecoder;   /* opaque */
/* parameters: diffusers' keys (decoder.conv_in.*, decoder.mid_block.resnets.{j}.{spatial_res_block,temporal_res_block}.*,
   decoder.mid_block.resnets.{j}.time_mixer.mix_factor, decoder.mid_block.attentions.0.*, decoder.up_blocks.{i}.resnets.{j}.* likewise,
   decoder.up_blocks.{i}.upsamplers.0.conv.*, decoder.conv_norm_out.*, decoder.conv_out.*, decoder.time_conv_out.*) */
int ctrl_vae_tdecoder_param_count(const ctrl_vae_decoder_config* cfg);
int ctrl_vae_tdecoder_param_spec(const ctrl_vae_decoder_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_vae_tdecoder_create(const ctrl_vae_decoder_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream,
                             ctrl_vae_tdecoder** out);
void ctrl_vae_tdecoder_destroy(ctrl_vae_tdecoder* h);
/* latents: `clips` clips of `num_frames` frames, frame (b, f) = image b * num_frames + f of the strided layout of
   ctrl_vae_decoder_forward_strided ([latent_channels][h][w] planes channel_stride apart, images image_stride apart), multiplied by
   `scale` on load; out: the clips' frames in the same order, the epilogue `kind` (CTRL_VAE_DEC_*) per frame.  Clips are decoded one
   after the other (a clip's pixels are bit-identical whatever else is in the call); inside a clip the launches run over groups of
   consecutive frames: frames_per_launch = 0 takes the largest group whose operands stay below 2^31 elements, a positive value caps
   it (the result is the same up to the GEMM tiles' summation order).  The first forward of a larger (size, frames) allocates the
   workspace (not under stream capture); every later one is capturable. */
int ctrl_vae_tdecoder_forward(ctrl_vae_tdecoder* h, const void* latents, int latent_dtype, int clips, int num_frames, int lat_h, int lat_w,
                              int64_t image_stride, int64_t channel_stride, float scale, int kind, void* out, int out_dtype,
                              int frames_per_launch, void* stream);
/* op level (csrc/vae.hip): time_conv_out of one clip.  x fp32 NCHW [F][Cout][H][W] (ctrl_op_vae_dec_tail's SAMPLE / fp32 frames) ->
   Conv3d (3,1,1), zero frames outside [0, F) (w fp32 [Cout][Cout][3], b [Cout], Cout <= 4), fp32 -> the epilogue `kind` over the F
   frames. */
int ctrl_op_vae_time_conv(const float* x, const float* w, const float* b, int F, int H, int W, int Cout, int kind, void* out,
                          int out_dtype, void* stream);

/* ---- HED annotator (controlnet_aux ControlNetHED_Apache2 + HEDdetector): the reference's `scribble` condition
 * (model/ctrl_helper.py:124-127, 196-197: HEDdetector(img, scribble=True)) and ControlNet's soft-edge condition (scribble = 0) ----
 * Parameters by controlnet_aux's state-dict keys: norm [1][3][1][1], blockK.convs.J.weight / .bias (K = 1..5; 2, 2, 3, 3, 3 convs of
 * 64, 128, 256, 512, 512 channels), blockK.projection.weight [1][C][1][1] / .bias [1].
 *   trunk_scale  a power of two s (default 1): the trunk runs on s * activations -- the stem multiplies (x - norm) by s, every trunk bias
 *                is multiplied by s once at creation, every projection multiplies by 1 / s before its bias; exact in the fp32
 *                accumulators, it moves the fp16 activations of a checkpoint with large activations (the input is 0..255) back into
 *                range.  A forward whose activations leave the fp16 range anyway returns an error (it reads one flag word back at
 *                its end, so it synchronises its stream and refuses a capturing one).
 *   ws_cap_bytes the workspace one group of frames may take (0 = 1 GiB): the frames of a call run in equal groups of the largest size
 *                that stays below it (one 512 x 512 frame needs about 70 MB), or in groups of frames_per_group when that is positive.
 *                A frame's result does not depend on the group it ran in.
 * ctrl_hed_forward: frames uint8 [N][H][W][3] (device), H and W multiples of 64 -> out uint8 [N][H][W] (out_channels 1) or
 * [N][H][W][3]: the soft edge map, or with scribble != 0 the map after nms(127, 3.0), GaussianBlur(sigma 3) and the binarisation;
 * logits (optional, device fp32 [N][H][W]): the mean of the five resized side outputs in front of the sigmoid.
 * ctrl_hed_ws_bytes: the workspace that forward would reserve (0 for arguments it would refuse). */
typedef struct ctrl_hed_config {
    float trunk_scale;
    int32_t reserved;
    int64_t ws_cap_bytes;
} ctrl_hed_config;
typedef struct ctrl_hed ctrl_hed;   /* opaque */
int ctrl_hed_create(const ctrl_hed_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_hed** out);
void ctrl_hed_destroy(ctrl_hed* h);
int ctrl_hed_forward(ctrl_hed* h, const void* frames_u8, int N, int H, int W, int scribble, int out_channels, void* out_u8, float* logits,
                     int frames_per_group, void* stream);
int64_t ctrl_hed_ws_bytes(ctrl_hed* h, int N, int H, int W, int scribble, int frames_per_group);
/* op level (csrc/hed.hip), the kernels around the trunk's implicit GEMMs (ctrl_igemm_desc::act = 3):
 *   stem       src uint8 [N][H][W][3] -> relu(conv3x3((x - norm) * scale, w) + bias) fp16 [N][H][W][64]; w fp32 [9][3][64]
 *              (ctrl_op_pack_conv_w_direct), bias fp32 [64] as it is added (the plan hands in scale * bias), norm: three floats on the
 *              HOST; the zero padding applies to x - norm; nonfinite (optional, device): set to 1 when an output leaves fp16; W % 4 == 0
 *   pool_proj  h fp16 [N][H][W][C] (C = 64 | 128 | 256 | 512, H and W even) -> p fp32 [N][H][W] = inv_scale * (h . wp) + bp[0] and,
 *              when pooled is not NULL, max_pool2d(h, 2, 2) fp16 [N][H/2][W/2][C]; wp fp32 [C], bp fp32 [1] (device)
 *   fuse       maps: HOST array of five device pointers, map k fp32 [N][H >> k][W >> k] -> cv2.resize(INTER_LINEAR) to H x W (float32,
 *              fx = (dx + 0.5) * scale - 0.5, clamped at both borders, rows interpolated along x first), the mean of the five (logits,
 *              optional fp32 [N][H][W]), uint8(clip(sigmoid * 255)) by truncation into out [N][H][W] | [N][H][W][3]; H, W % 16 == 0
 *   blur_f32   uint8 [N][H][W] -> fp32: cv2.GaussianBlur(x.astype(float32), (0, 0), 3.0), 25 taps, BORDER_REFLECT_101
 *   nms        fp32 [N][H][W] -> uint8: 255 where cv2.dilate(x, f) == x for one of the four 3-pixel line kernels and x > 127, else 0
 *   blur_u8_bin uint8 [N][H][W] -> cv2.GaussianBlur(x, (0, 0), 3.0) on uint8 (19 taps), then > 4 -> 255, else 0, on out_channels channels
 * The three tail kernels reproduce tests/hed_ref.py bit for bit: taps normalised in double and cast to float, every tap one rounded
 * multiply and one rounded add in fp32 from left to right, the row pass before the column pass. */
int ctrl_op_hed_stem(const void* src_u8, int N, int H, int W, const float* w, const float* bias, const float* norm_host3, float scale,
                     void* out_f16, int32_t* nonfinite, void* stream);
int ctrl_op_hed_pool_proj(const void* h_f16, int N, int H, int W, int C, const float* wp, const float* bp, float inv_scale, void* pooled_f16,
                          float* p, void* stream);
int ctrl_op_hed_fuse(const float* const* maps, int N, int H, int W, int out_channels, void* out_u8, float* logits, void* stream);
int ctrl_op_hed_blur_f32(const void* src_u8, int N, int H, int W, float* out, void* stream);
int ctrl_op_hed_nms(const float* x, int N, int H, int W, void* out_u8, void* stream);
int ctrl_op_hed_blur_u8_bin(const void* src_u8, int N, int H, int W, int out_channels, void* out_u8, void* stream);

/* ---- PiDiNet annotator (controlnet_aux PidiNetDetector, pidinet() = PiDiNet(60, 'carv4', dil 24, sa)): the reference's `softedge`
 * condition (model/ctrl_helper.py:103-107, 184-185) ----
 * Parameters by the checkpoint's keys with `module.` stripped: init_block.weight [60][3][3][3], block{s}_{j}.conv1.weight [C][1][3][3],
 * .conv2.weight [Co][C][1][1], .shortcut.weight [Co][C][1][1] / .bias [Co] (the first block of stages 2, 3, 4),
 * dilations.{i}.conv1.weight [24][C][1][1] / .bias, .conv2_{1..4}.weight [24][24][3][3], attentions.{i}.conv1.weight [4][24][1][1] / .bias,
 * .conv2.weight [1][4][3][3], conv_reduces.{i}.conv.weight [1][24][1][1] / .bias, classifier.weight [1][4][1][1] / .bias.
 * Activations are fp16 NHWC with the channels padded 60 -> 64, 120 -> 128, 240 -> 256 (pad channels hold exact zeros); a forward in which
 * a stored activation leaves the fp16 range returns an error (it reads one flag word back: it synchronises and refuses a capturing stream).
 *   ws_cap_bytes      the workspace one group of frames may take (0 = 1 GiB); frames_per_group > 0 fixes the group instead (the
 *                     forward's own argument, when positive, wins).  A frame's result does not depend on its batch or group.
 * ctrl_pidi_forward: frames uint8 [N][H][W][3] RGB (device), H and W multiples of 64 -> out uint8 [N][H][W] | [N][H][W][3]: the soft edge
 * map (apply_filter: 255 where the edge is > 0.5, else 0), with scribble != 0 HED's tail behind it; logits (optional, fp32 [N][H][W]): the
 * classifier's output in front of the sigmoid. */
typedef struct ctrl_pidi_config {
    int32_t frames_per_group;
    int32_t reserved;
    int64_t ws_cap_bytes;
} ctrl_pidi_config;
typedef struct ctrl_pidi ctrl_pidi;   /* opaque */
int ctrl_pidi_create(const ctrl_pidi_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_pidi** out);
void ctrl_pidi_destroy(ctrl_pidi* h);
int ctrl_pidi_forward(ctrl_pidi* h, const void* frames_u8, int N, int H, int W, int scribble, int apply_filter, int out_channels, void* out_u8,
                      float* logits, int frames_per_group, void* stream);
int64_t ctrl_pidi_ws_bytes(ctrl_pidi* h, int N, int H, int W, int scribble, int frames_per_group);
/* HOST only.  convert_pdc: a pixel-difference convolution's weight w fp32 [Co][Ci][3][3] -> the vanilla kernel that computes the same
 * map, out fp32 [Co][Ci][9] (kind 0 cv, 1 cd, 2 ad) or [Co][Ci][25] (kind 3 rd); computed in double, rounded once.
 * launch_shape: the output tile (pixels) one workgroup owns, kernel 0 = the PDC block, 1 = the context head. */
int ctrl_pidi_convert_pdc(int kind, const float* w, int Co, int Ci, float* out);
int ctrl_pidi_launch_shape(int kernel, int* tile_h, int* tile_w);
/* op level (csrc/pidinet.hip).  CP(C) = C rounded up to 64; every weight below is padded with zeros to these widths.
 *   stem       src uint8 [N][H][W][3] RGB -> conv3x3(BGR / 255, w) fp16 [N][H][W][64]; w fp32 [9][3][64], tap-major, channel index in the
 *              NET's (BGR) order; W % 4 == 0
 *   block      x fp16 [N][H][W][CP(Cin)] -> out fp16 [N][Ho][Wo][CP(Cout)] = conv2(relu(dw(xp))) + skip, xp = x (pool 0, Ho = H) or
 *              max_pool2d(x, 2, 2) (pool 1, Ho = H / 2); dw fp32 [taps][CP(Cin)], taps 9 (3 x 3) or 25 (the rd footprint: the nine
 *              positions convert_pdc leaves zero are not read); w2 fp16 [CP(Cout)][CP(Cin)]; skip = xp (wsc NULL; Cin == Cout) or
 *              wsc . xp + bsc (wsc fp16 [CP(Cout)][CP(Cin)], bsc fp32 [CP(Cout)]).  The input's pad channels are not read as values.
 *   head_reduce   t fp16 [N][H][W][32] = w1 . relu(x) + b1; w1 fp16 [32][CP(C)], b1 fp32 [32] (rows 24..31 zero)
 *   head_context  s = the sum of the four dilated 3 x 3 convolutions of t (wd fp16 [36][32][32]: [dilation 5,7,9,11][ky][kx] x cout x cin),
 *              kept in fp32; a4 fp32 [N][H][W][4] = att . relu(s) + att_b, d fp32 [N][H][W] = red . s; par: HOST fp32 [124] =
 *              att [4][24] | att_b [4] | red [24]
 *   side       e fp32 [N][H][W] = sigmoid(conv3x3(a4, w)) * d + b; par: HOST fp32 [37] = w [ky][kx][4] | b
 *   fuse       maps: HOST array of four device pointers, map k fp32 [N][H >> k][W >> k] -> torch's bilinear (align_corners = False) to
 *              H x W, logit = cls . e + cls_b (par: HOST fp32 [5]), sigmoid, apply_filter, * 255, clip, truncation; H, W % 8 == 0 */
int ctrl_op_pidi_stem(const void* src_u8, int N, int H, int W, const float* w, void* out_f16, int32_t* nonfinite, void* stream);
int ctrl_op_pidi_block(const void* x_f16, int N, int H, int W, int Cin, int Cout, int taps, const float* dw, const void* w2_f16,
                       const void* wsc_f16, const float* bsc, int pool, void* out_f16, int32_t* nonfinite, void* stream);
int ctrl_op_pidi_head_reduce(const void* x_f16, int N, int H, int W, int C, const void* w1_f16, const float* b1, void* t_f16,
                             int32_t* nonfinite, void* stream);
int ctrl_op_pidi_head_context(const void* t_f16, int N, int H, int W, const void* wd_f16, const float* par_host124, float* a4, float* d,
                              void* stream);
int ctrl_op_pidi_side(const float* a4, const float* d, int N, int H, int W, const float* par_host37, float* e, void* stream);
int ctrl_op_pidi_fuse(const float* const* maps, int N, int H, int W, const float* par_host5, int apply_filter, int out_channels,
                      void* out_u8, float* logits, void* stream);

/* ---- Lineart annotator (controlnet_aux LineartDetector: two Generator(3, 1, 3) nets, sk_model.pth and sk_model2.pth for coarse): the
 * reference's `lineart` condition (model/ctrl_helper.py:111-114, 190-191) ----
 * Parameters by the checkpoints' keys under the prefix `fine.` (and `coarse.` when has_coarse != 0), weight and bias each:
 * model0.1 [64][3][7][7], model1.0 [128][64][3][3], model1.3 [256][128][3][3], model2.{0,1,2}.conv_block.{1,5} [256][256][3][3],
 * model3.0 [256][128][3][3] and model3.3 [128][64][3][3] (ConvTranspose2d: [Cin][Cout][3][3]), model4.1 [1][64][7][7].  Every norm is
 * InstanceNorm2d without affine parameters (eps 1e-5, biased variance), so every bias but model4.1's cancels and is dropped at load; all
 * of them must still be present and well-shaped.  Activations are fp16 NHWC; a forward in which a stored activation leaves the fp16 range
 * returns an error (it reads one flag word back: it synchronises and refuses a capturing stream).
 *   ws_cap_bytes      the workspace one group of frames may take (0 = 1 GiB; one 512 x 512 frame needs about 105 MB); frames_per_group > 0
 *                     fixes the group instead (the forward's own argument, when positive, wins).  A frame's result does not depend on its
 *                     batch or group.
 * ctrl_lineart_forward: frames uint8 [N][H][W][3] RGB (device), H and W multiples of 64 -> out uint8 [N][H][W] | [N][H][W][3]:
 * 255 - uint8(clip(255 sigmoid(logit))) (truncation); coarse != 0 runs the coarse generator; logits (optional, fp32 [N][H][W]): model4.1's
 * output in front of the sigmoid. */
typedef struct ctrl_lineart_config {
    int32_t frames_per_group;
    int32_t has_coarse;
    int64_t ws_cap_bytes;
} ctrl_lineart_config;
typedef struct ctrl_lineart ctrl_lineart;   /* opaque */
int ctrl_lineart_create(const ctrl_lineart_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_lineart** out);
void ctrl_lineart_destroy(ctrl_lineart* h);
int ctrl_lineart_forward(ctrl_lineart* h, const void* frames_u8, int N, int H, int W, int coarse, int out_channels, void* out_u8, float* logits,
                         int frames_per_group, void* stream);
int64_t ctrl_lineart_ws_bytes(ctrl_lineart* h, int N, int H, int W, int frames_per_group);
/* HOST only.  kernel 0 (stem) and 1 (head): the output tile one workgroup owns, *a rows by *b columns; kernel 2 (in_stats): *a = the rows
 * of an image one workgroup reduces for maps of C channels, *b = 1. */
int ctrl_lineart_launch_shape(int kernel, int C, int* a, int* b);
/* op level (csrc/lineart.hip).
 *   stem       src uint8 [N][H][W][3] RGB -> conv7x7(reflect_pad3(x / 255), w) fp16 [N][H][W][64]; w fp32 [49][3][64] (tap-major: ky, kx,
 *              then the input channel); no bias; H, W >= 4
 *   in_stats   x fp16 [N][HW][C] (C = 8 .. 256, a power of two) -> stats fp32 [N][C][2] = (sum, sum of squares) over the HW rows, in a
 *              fixed order; ws: ctrl_op_in_stats_ws_floats(N, HW, C) floats of scratch
 *   in_apply   y = (x - mean) * rsqrt(var + eps), mean = sum / HW, var = max(sumsq / HW - mean^2, 0); ReLU when relu != 0; + res when
 *              given; out fp16 [N][H + 2 pad][W + 2 pad][C], pad 0 | 1 | 3: the map with its reflection padding (no edge repeat)
 *              written out; res fp16 [N][H + 2 res_pad][W + 2 res_pad][C] is read at its interior
 *   head       xp fp16 [N][H + 6][W + 6][64] (reflect-padded by 3) -> logit = conv7x7(xp, w) + bias (w fp32 [49][64], tap-major) ->
 *              out uint8 [N][H][W] | [N][H][W][3] = 255 - uint8(min(255, 255 sigmoid(logit))); logits (optional) fp32 [N][H][W]
 *   pack_convT_w_phase  ConvTranspose2d(3, stride 2, padding 1, output_padding 1) weight [Cin][Cout][3][3] (any dtype) -> fp16
 *              [4][Cout][4][Cin], the weight pack of ctrl_igemm_desc::mode 3: phase 2a + b, tap 2ty + tx takes w[ci][co][ky][kx] with
 *              (a, ty) -> ky: (0,0) none (zero), (0,1) 1, (1,0) 2, (1,1) 0 and the same for (b, tx) -> kx; _ovf also raises *ovf (device)
 *              when a value does not fit fp16 */
int ctrl_op_lineart_stem(const void* src_u8, int N, int H, int W, const float* w, void* out_f16, int32_t* nonfinite, void* stream);
int64_t ctrl_op_in_stats_ws_floats(int N, int HW, int C);
int ctrl_op_in_stats(const void* x_f16, int N, int HW, int C, float* stats, float* ws, void* stream);
int ctrl_op_in_apply(const void* x_f16, const float* stats, int N, int H, int W, int C, float eps, int relu, const void* res_f16, int res_pad,
                     int pad, void* out_f16, int32_t* nonfinite, void* stream);
int ctrl_op_lineart_head(const void* xp_f16, int N, int H, int W, const float* w, float bias, int out_channels, void* out_u8, float* logits,
                         void* stream);
int ctrl_op_pack_convt_w_phase(const void* w, int dtype, void* out, int Cin, int Cout, void* stream);
int ctrl_op_pack_convt_w_phase_ovf(const void* w, int dtype, void* out, int Cin, int Cout, int32_t* ovf, void* stream);

/* ---- SVD backbone UNet(diffusers UNetSpatioTemporalConditionModel with the reference's two ControlNet-residual kwargs) ---- */
typedef struct ctrl_unet_st_config {
    int32_t in_channels;                           /* 8 */
    int32_t out_channels;                          /* 1..4 */
    int32_t num_levels;                            /* len(block_out_channels), 1..4 */
    int32_t block_out_channels[4];                 /* multiples of 64 */
    int32_t layers_per_block;                      /* down blocks hold this many ResNets, up blocks one more */
    int32_t transformer_layers_per_block;
    int32_t num_attention_heads[4];                /* per level; out_channels / heads must be 64 where the level (or the mid block) attends */
    int32_t cross_attention_dim;
    int32_t level_has_attn[4];                     /* down block i is CrossAttnDownBlockSpatioTemporal (up block levels-1-i mirrors it) */
    int32_t addition_time_embed_dim;
    int32_t projection_class_embeddings_input_dim;
} ctrl_unet_st_config;
typedef struct ctrl_unet_st ctrl_unet_st;   /* opaque */
/* parameters: diffusers' keys (conv_in.*, time_embedding.linear_{1,2}.*, add_embedding.linear_{1,2}.*,
   {down,up}_blocks.{i}.resnets.{j}.{spatial_res_block,temporal_res_block}.*, ....resnets.{j}.time_mixer.mix_factor,
   ....attentions.{j}.{norm,proj_in,proj_out}.*, ....attentions.{j}.time_pos_embed.linear_{1,2}.*, ....attentions.{j}.time_mixer.mix_factor,
   ....attentions.{j}.transformer_blocks.{k}.*, ....attentions.{j}.temporal_transformer_blocks.{k}.*, ....downsamplers.0.conv.*,
   ....upsamplers.0.conv.*, mid_block.*, conv_norm_out.*, conv_out.*) */
int ctrl_unet_st_param_count(const ctrl_unet_st_config* cfg);
int ctrl_unet_st_param_spec(const ctrl_unet_st_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_unet_st_create(const ctrl_unet_st_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet_st** out);
void ctrl_unet_st_destroy(ctrl_unet_st* h);
/* what plan creation selected, as one text line */
int ctrl_unet_st_selection(ctrl_unet_st* h, char* buf, int len);
/* sample [B][F][in_channels][h][w] (CTRL_F32 / F16 / BF16) -> out [B][F][out_channels][h][w] in the same dtype.  timesteps: fp32 device,
   1 or B values; encoder_hidden_states [B][1][cross_attention_dim] (one key); added_time_ids fp32 device [B][n_time_ids].
   down_residuals (host array of n_down_residuals device pointers, may be 0): residual i is added to skip i -- skip 0 is conv_in's output,
   then every down block's ResNet / transformer outputs and its down-sampler's -- all in one dtype and one layout: (b f) c h w
   (down_5d = 0) or b c f h w (down_5d = 1).  mid_residual (may be NULL) likewise, added to the mid block's output.  h and w must be
   multiples of 2^(num_levels - 1), F <= 32.  The first forward of a larger size allocates the workspace (not under stream capture);
   every later one is capturable: one stream, no side lanes. */
int ctrl_unet_st_forward(ctrl_unet_st* h, const void* sample, int sample_dtype, int B, int F, int lat_h, int lat_w, const float* timesteps,
                         int t_count, const void* encoder_hidden_states, int ehs_dtype, const float* added_time_ids, int n_time_ids,
                         const void* const* down_residuals, int n_down_residuals, int down_dtype, int down_5d, const void* mid_residual,
                         int mid_dtype, int mid_5d, void* out, void* stream);
/* op level (csrc/unet.hip): one skip tensor of the up path.  out32[r][col + c] = skip[r][c] (+ res(b, f, c, p)) for the B * F * HW rows
   r = (b F + f) HW + p and c < C2 (a multiple of 32), and out16 (may be NULL) its fp16 rounding; skip rows ld_skip floats apart, out rows
   ld_out elements.  res (may be NULL): (b f) c h w (res_5d = 0) or b c f h w (res_5d = 1) in res_dtype.  skip may be out32 with col = 0. */
int ctrl_op_unet_skip_join(const float* skip, int64_t ld_skip, const void* res, int res_dtype, int res_5d, int B, int F, int HW, int C2,
                           float* out32, void* out16, int64_t ld_out, int col, void* stream);
/* Test ABI (tests/shell_forms.py, tests/test_gpu_shell_forms.py): the form the SDXL and I2VGen-XL plans launch.
   The same with a split mirror (lo_off != 0; lo_off = 0 is the call above): out16 rows are 2 * ld_out halves wide, hi = fp16(v) at
   [col, col + C2) and lo = fp16(v - hi) at lo_off + [col, col + C2).  lo_off a multiple of 8, at least col + C2, lo_off + col + C2 <=
   2 * ld_out; needs out16. */
int ctrl_op_unet_skip_join_split(const float* skip, int64_t ld_skip, const void* res, int res_dtype, int res_5d, int B, int F, int HW, int C2,
                                 float* out32, void* out16, int64_t ld_out, int col, int lo_off, void* stream);

/* ---- SDXL backbone UNet (diffusers UNet2DConditionModel, addition_embed_type "text_time", linear transformer projections) ---- */
typedef struct ctrl_unet2d_config {
    int32_t in_channels;                           /* 4 or 8 (the stem kernel's instantiations) */
    int32_t out_channels;                          /* 1..4 */
    int32_t num_levels;                            /* len(block_out_channels), 1..4 */
    int32_t block_out_channels[4];                 /* multiples of 64 */
    int32_t layers_per_block;                      /* down blocks hold this many ResNets, up blocks one more */
    int32_t transformer_layers_per_block[4];       /* per level; the mid block takes the last level's, up block i level (levels-1-i)'s */
    int32_t num_attention_heads[4];                /* per level; out_channels / heads must be 64 where the level (or the mid block) attends */
    int32_t cross_attention_dim;
    int32_t level_has_attn[4];                     /* down block i is CrossAttnDownBlock2D (up block levels-1-i mirrors it) */
    int32_t addition_time_embed_dim;
    int32_t projection_class_embeddings_input_dim; /* text_embeds width + n_time_ids * addition_time_embed_dim */
    float norm_eps;                                /* the ResNets' and conv_norm_out's GroupNorm eps */
} ctrl_unet2d_config;
typedef struct ctrl_unet2d ctrl_unet2d;   /* opaque */
/* parameters: diffusers' keys (conv_in.*, time_embedding.linear_{1,2}.*, add_embedding.linear_{1,2}.*, {down,up}_blocks.{i}.resnets.{j}.*,
   ....attentions.{j}.{norm,proj_in,proj_out}.*, ....attentions.{j}.transformer_blocks.{k}.*, ....downsamplers.0.conv.*,
   ....upsamplers.0.conv.*, mid_block.{resnets,attentions}.*, conv_norm_out.*, conv_out.*) */
int ctrl_unet2d_param_count(const ctrl_unet2d_config* cfg);
int ctrl_unet2d_param_spec(const ctrl_unet2d_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_unet2d_create(const ctrl_unet2d_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet2d** out);
void ctrl_unet2d_destroy(ctrl_unet2d* h);
/* what plan creation selected, as one text line */
int ctrl_unet2d_selection(ctrl_unet2d* h, char* buf, int len);
/* step-invariant cache of the text K / V^T projections of every cross-attention: mode 0 off, 1 keep (this forward fills the plan-owned
   buffers; the first one of a shape allocates them: not under stream capture), 2 reuse (the projections are skipped) */
int ctrl_unet2d_set_text_cache(ctrl_unet2d* h, int mode);
/* sample [B][in_channels][h][w] (CTRL_F32 / F16 / BF16) -> out [B][out_channels][h][w] in the same dtype.  timesteps: fp32 device, 1 or B
   values; encoder_hidden_states [B][Lk][cross_attention_dim]; text_embeds [B][text_dim] (any of the three dtypes) and time_ids fp32
   device [B][n_time_ids], with text_dim + n_time_ids * addition_time_embed_dim == projection_class_embeddings_input_dim.
   down_residuals (host array of n_down_residuals device pointers, may be 0): residual i, b c h w in down_dtype, is added to skip i --
   skip 0 is conv_in's output, then every down block's layer outputs and its down-sampler's.  mid_residual (may be NULL) likewise, added
   to the mid block's output.  h and w must be multiples of 2^(num_levels - 1).  The first forward of a larger size allocates the
   workspace (not under stream capture); every later one is capturable: one stream, no side lanes. */
int ctrl_unet2d_forward(ctrl_unet2d* h, const void* sample, int sample_dtype, int B, int lat_h, int lat_w, const float* timesteps,
                        int t_count, const void* encoder_hidden_states, int ehs_dtype, int Lk, const void* text_embeds, int text_dtype,
                        int text_dim, const float* time_ids, int n_time_ids, const void* const* down_residuals, int n_down_residuals,
                        int down_dtype, const void* mid_residual, int mid_dtype, void* out, void* stream);
/* bytes of the plan's forward workspace (the largest forward so far) */
int64_t ctrl_unet2d_workspace_bytes(ctrl_unet2d* h);
/* op level (csrc/unet.hip): the operand rows of add_embedding.linear_1.  out fp32 [B][ld_out >= text_dim + n_ids * dim]:
   columns [0, text_dim) = text_embeds[b] converted to fp32, columns text_dim + i * dim + [0, dim) = the sinusoidal embedding of
   time_ids[b][i] (flip_sin_to_cos, shift 0: [cos | sin], ctrl_op_timestep_sincos's arithmetic).  dim even. */
int ctrl_op_unet_text_time(const void* text_embeds, int text_dtype, int text_dim, const float* time_ids, int n_ids, int dim, float* out,
                           int64_t ld_out, int B, void* stream);

/* ---- I2VGen-XL backbone UNet (I2VGenXLUNet with the reference's two ControlNet-residual kwargs; diffusers' 3D blocks) ---- */
typedef struct ctrl_unet_i2v_config {
    int32_t in_channels;                           /* 4 */
    int32_t out_channels;                          /* 1..4 */
    int32_t num_levels;                            /* len(block_out_channels), 1..4 */
    int32_t block_out_channels[4];                 /* multiples of 64: every transformer of a level has out_channels / 64 heads of 64 */
    int32_t layers_per_block;                      /* down blocks hold this many layers, up blocks one more */
    int32_t cross_attention_dim;                   /* a multiple of 32 */
    int32_t level_has_attn[4];                     /* down block i is CrossAttnDownBlock3D (up block levels-1-i mirrors it) */
} ctrl_unet_i2v_config;
typedef struct ctrl_unet_i2v ctrl_unet_i2v;   /* opaque */
/* parameters: the reference's keys (conv_in.*, transformer_in.*, image_latents_proj_in.{0,2,4}.*, image_latents_temporal_encoder.*,
   image_latents_context_embedding.{0,3,5}.*, time_embedding.linear_{1,2}.*, context_embedding.{0,2}.*, fps_embedding.{0,2}.*,
   {down,up}_blocks.{i}.{resnets,temp_convs,attentions,temp_attentions}.{j}.*, ....downsamplers.0.conv.*, ....upsamplers.0.conv.*,
   mid_block.*, conv_norm_out.*, conv_out.*) */
int ctrl_unet_i2v_param_count(const ctrl_unet_i2v_config* cfg);
int ctrl_unet_i2v_param_spec(const ctrl_unet_i2v_config* cfg, int i, char* name, int name_len, int64_t shape[6], int* ndim);
int ctrl_unet_i2v_create(const ctrl_unet_i2v_config* cfg, const ctrl_tensor_ref* tensors, int n_tensors, void* stream, ctrl_unet_i2v** out);
void ctrl_unet_i2v_destroy(ctrl_unet_i2v* h);
/* what plan creation selected, as one text line */
int ctrl_unet_i2v_selection(ctrl_unet_i2v* h, char* buf, int len);
/* step-invariant cache of everything that depends on encoder_hidden_states, image_latents and image_embeddings only -- the context
   matrix's K / V^T projections of every cross-attention and the four encoded latent channels: mode 0 off, 1 keep (this forward fills
   the plan-owned buffers; the first one of a shape allocates them: not under stream capture), 2 reuse (the stems and the projections
   are skipped; the three condition inputs are not read) */
int ctrl_unet_i2v_set_cond_cache(ctrl_unet_i2v* h, int mode);
/* sample [B][in_channels][F][h][w] (CTRL_F32 / F16 / BF16) -> out [B][out_channels][F][h][w] in the same dtype.  timesteps and fps: fp32
   device, 1 or B values each; image_latents [B][4][F][h][w], image_embeddings [B][cross_attention_dim], encoder_hidden_states
   [B][text_len][cross_attention_dim], each in any of the three dtypes.  down_residuals (host array of n_down_residuals device pointers,
   may be 0): residual i is added to skip i -- skip 0 is transformer_in's output, then every down block's layer outputs and its
   down-sampler's -- all in one dtype and one layout: (b f) c h w (down_5d = 0) or b c f h w (down_5d = 1).  mid_residual (may be NULL)
   likewise, added to the mid block's output.  h and w must be multiples of 2^(num_levels - 1), F <= 32.  The first forward of a larger
   size allocates the workspace (not under stream capture); every later one is capturable: one stream, no side lanes. */
int ctrl_unet_i2v_forward(ctrl_unet_i2v* h, const void* sample, int sample_dtype, int B, int F, int lat_h, int lat_w, const float* timesteps,
                          int t_count, const float* fps, int fps_count, const void* image_latents, int latents_dtype,
                          const void* image_embeddings, int embeddings_dtype, const void* encoder_hidden_states, int ehs_dtype, int text_len,
                          const void* const* down_residuals, int n_down_residuals, int down_dtype, int down_5d, const void* mid_residual,
                          int mid_dtype, int mid_5d, void* out, void* stream);
/* bytes of the plan's forward workspace (the largest forward so far) */
int64_t ctrl_unet_i2v_workspace_bytes(ctrl_unet_i2v* h);
/* op level (csrc/unet.hip): I2VGenXLTransformerTemporalEncoder with dim 4 (LayerNorm, two heads of 4 over the F <= 32 frames of a pixel,
   to_out + residual, feed-forward 4 -> 16 -> 4 with erf GELU + residual), fp32 throughout, one launch.  x fp32 rows [(b f) HW][4] ->
   columns 4..7 of out8, fp32 rows [(b f) HW][8]; sample (may be NULL) [B][4][F][HW] in sample_dtype -> columns 0..3, converted once; keep
   (may be NULL) fp32 [(b f) HW][4] receives the encoded rows once more.  weights: 288 floats, norm1 weight[4] bias[4] | to_q [8][4] |
   to_k [8][4] | to_v [8][4] | to_out.0 weight [4][8] bias[4] | ff.net.0.proj weight [16][4] bias[16] | ff.net.2 weight [4][16] bias[4].
   precomputed = 1: x already holds encoded rows, which are copied (weights may be NULL). */
int ctrl_op_i2v_latent_encoder(const float* x, const float* weights, const void* sample, int sample_dtype, float* out8, float* keep, int B,
                               int F, int HW, int precomputed, void* stream);
/* op level (csrc/unet.hip): adaptive_avg_pool2d of a channels-last map x [N][H][W][C] to y [N][OH][OW][C] (each CTRL_F32 or CTRL_F16):
   output (i, j) is the mean over rows [floor(i H / OH), ceil((i + 1) H / OH)) and the like columns, summed in fp32 */
int ctrl_op_adaptive_avgpool_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int N, int H, int W, int C, int OH, int OW, void* stream);

/* ---- Samplers (csrc/sampler.hip, csrc/plan_sampler.cpp): the per-step glue of a denoise loop ---- */
/* One scheduler step of every supported sampler (Euler, DDIM; eta = 0) is linear in the sample x and the guided model output m:
   prev = A_i x + B_i m, and the model eats c_i x.  The host computes the table in fp64 and hands it over as fp32 rows of
   CTRL_SAMPLER_ROW floats, one per step: { c_in, A, B, t_model, t_aux0, t_aux1, 0, 0 }.  The kernels multiply and add, nothing else. */
#define CTRL_SAMPLER_ROW 8
typedef struct ctrl_sampler_desc {
    const void* x;          /* latents, (outer, C, inner) dense, x_dtype */
    void* prev;             /* step: A x + B mg, same shape, prev_dtype; may be x itself (then prev_dtype == x_dtype) */
    const void* model_out;  /* step: (R * outer, C, inner) in mo_dtype, the unconditional replica first */
    const float* g;         /* step, R = 2: guidance per frame, fp32 device [g_count]; NULL = g_scalar */
    void* unet_in;          /* model input: (R * outer, C + C2, inner) in unet_dtype = round(c_in * latents), R replicas along outer */
    const void* concat;     /* model input: (R * outer, C2, inner) in concat_dtype, copied behind the C channels (NULL: C2 = 0) */
    void* cn_in;            /* model input (may be NULL): the scaled, replicated latents once more without the concat, in cn_dtype */
    int32_t x_dtype, prev_dtype, mo_dtype, unet_dtype, concat_dtype, cn_dtype;
    int32_t outer, C, inner, C2;
    int32_t R;              /* 1 | 2 classifier-free-guidance replicas */
    int32_t cn_frames;      /* 0: cn_in is laid out as the latents; F > 0: inner = F * hw and cn_in is (R * outer * F, C, hw), the
                               b c f h w -> (b f) c h w rearrange */
    int32_t g_count, g_inner;   /* element e of the latents takes g[(e / g_inner) % g_count] */
    float g_scalar;
    int32_t pad0_;
} ctrl_sampler_desc;
typedef struct ctrl_sampler ctrl_sampler;   /* opaque: the device table, the step counter (+ its ticket word) and three scalars */
/* table_fp32_host: n_steps rows; created on the current device (a synchronous upload) */
int ctrl_sampler_create(int n_steps, const float* table_fp32_host, ctrl_sampler** out);
void ctrl_sampler_destroy(ctrl_sampler* h);
/* step counter = 0, by a one-thread kernel (capturable) */
int ctrl_sampler_reset(ctrl_sampler* h, void* stream);
/* fp32 device [3]: t_model, t_aux0, t_aux1 of the row the last model-input pass used -- what the modules' `timesteps` (t_count = 1) read */
float* ctrl_sampler_scalars(ctrl_sampler* h);
/* the model's inputs of step `step_index` (>= 0; -1: the device counter, which is not advanced) from d->x; writes the scalars */
int ctrl_sampler_model_input(ctrl_sampler* h, const ctrl_sampler_desc* d, int step_index, void* stream);
/* prev = A_i x + B_i (u + g (c - u)) with row i = step_index (>= 0), or i = the device counter (-1), which the last workgroup of the
   launch to finish then advances.  prepare_next: the same launch writes what ctrl_sampler_model_input would write for step i + 1 from
   the rounded prev (bit-identical to the two calls; skipped on the last step).  A counter beyond the table makes the launch a no-op. */
int ctrl_sampler_step(ctrl_sampler* h, const ctrl_sampler_desc* d, int step_index, int prepare_next, void* stream);
/* op level: the same launches on caller-owned buffers.  table: fp32 device [n_steps][CTRL_SAMPLER_ROW]; counter: int32 device [2]
   (step, ticket), zero once (ctrl_op_sampler_reset zeroes both); scalars: fp32 device [3] */
int ctrl_op_sampler_reset(int32_t* counter, void* stream);
int ctrl_op_sampler_model_input(const float* table, int n_steps, const int32_t* counter, float* scalars, const ctrl_sampler_desc* d,
                                int step_index, void* stream);
int ctrl_op_sampler_step(const float* table, int n_steps, int32_t* counter, float* scalars, const ctrl_sampler_desc* d, int step_index,
                         int prepare_next, void* stream);
/* how a launch over `d` would run (host only): workgroups of 256 threads, elements per thread and access (8: 16-byte accesses, 1: the
   scalar path), and the cap on the grid beyond which the grid-stride loop takes further trips */
int ctrl_op_sampler_launch_shape(const ctrl_sampler_desc* d, int with_step, int with_model_input, int* blocks, int* vec, int* grid_cap);

/* ---- Router (model/ctrl_router.py) ---- */
/* weights_out fp32 device [num_routers + (has_mid?1:0)][E]; wg fp32 device same shape (Linear(1,E).weight[:,0]
 * per router; ignored for equal_weights); mask host int[E] (NULL = all ones). */
int ctrl_router_weights(const float* wg, const int* mask_host, float* weights_out, int R, int E,
                        int equal_weights, void* stream);
/* out = sum_k weights[row*E + widx[k]] * experts[k]  over K active experts, element-wise on n elements */
int ctrl_router_merge(const void* const* experts_host, const float* weights_row, const int* widx_host, int K,
                      void* out, int dtype, size_t n, void* stream);
/* Router merge, key-frame gather and cast of up to CTRL_MERGE_SLOTS slots (the 12 down residuals and the mid one) in ONE launch:
     out[s][j][i] = round_to_out_dtype( sum_{k < K} w[row_s * E + widx[k]] * in[k][s][ map[j] ][i] ),  j < n_out, i < elems_s
   summed in fp32 in expert order with ctrl_router_merge's expression (where the dtypes agree the result is bit-identical to
   ctrl_router_merge followed by an index_select).  w: fp32 device [R][E], the router's output, NULL = weight 1 (then K == 1: an exact
   gather + cast); widx: host int[K]; map: int32 device [n_out] frame indices into the n_in input frames, NULL = the identity
   (n_out == n_in); an entry outside [0, n_in) yields NaN frames.  in_dtype / out_dtype: CTRL_F32 / CTRL_F16 / CTRL_BF16, independent.
   The slot table travels in the kernel arguments: the host reads no device memory and does not synchronise, so the launch records
   into a graph.  Work is dealt out by elements (chunks of 256 threads x vec elements, prefix sums over the slots), 16-byte accesses
   when every elems_s is a multiple of 8 and every pointer 16-byte aligned, the scalar path otherwise. */
#define CTRL_MERGE_SLOTS 13
typedef struct ctrl_merge_slot {
    const void* in[8];      /* K expert tensors [n_in][elems], in_dtype */
    void* out;              /* [n_out][elems], out_dtype */
    int64_t elems;          /* elements of one frame */
    int32_t row;            /* row of w this slot reads */
    int32_t pad0_;
} ctrl_merge_slot;
int ctrl_op_merge_gather_group(const ctrl_merge_slot* slots, int n_slots, const float* w, int R, int E, const int* widx_host, int K,
                               const int32_t* map, int n_in, int n_out, int in_dtype, int out_dtype, void* stream);
/* how that launch would run (host only, the same argument checks): workgroups of 256 threads, elements per thread and access (8 | 1),
   and the cap on the grid beyond which the grid-stride loop takes further trips */
int ctrl_op_merge_gather_launch_shape(const ctrl_merge_slot* slots, int n_slots, const float* w, int R, int E, const int* widx_host, int K,
                                      const int32_t* map, int n_in, int n_out, int in_dtype, int out_dtype, int* blocks, int* vec,
                                      int* grid_cap);

#ifdef __cplusplus
}
#endif
#endif /* CTRL_HIP_H */
