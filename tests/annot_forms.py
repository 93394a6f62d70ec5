"""The condition path's memory-bound kernels at their quad and tile edges: the HED annotator's stem, pool + project, fuse and scribble tail
(csrc/hed.hip), the PiDiNet stem, side map and fuse (csrc/pidinet.hip) and the two image-preparation kernels (csrc/imageprep.hip).  Case
tables built from the kernels' tile constants, problem builders seeded by shape, the references of the older tests (tests/hed_ref.py,
tests/pidinet_ref.py, oracle/image_prep.py) with their bounds unchanged, restatements of the kernels' index arithmetic and the planted
errors the checks have to reject.  Pure data: imports no GPU code.

    GPU tests: tests/test_gpu_hed_forms.py, tests/test_gpu_prep_forms.py, tests/test_gpu_pidinet.py
    host self-test (no GPU): tests/test_annot_check_host.py

What is exact and what is bounded.
  stems       fp64 convolution; HED: helpers.igemm_bound with K = 28 (27 taps + the subtraction's rounding) and an fp16 store, as
              test_gpu_hed.py::test_stem; PiDiNet: pidinet_ref.stem_ref.  Every frame has the corner pixels 255 and 0.
  pool_proj   the projection: helpers.igemm_bound with K = C, fp32 store; the pooled map: bit for bit.
  HED fuse    hed_ref.resize_linear in fp64 with 16 * 2^-24 * mag on the logit, the byte inside hed_ref.u8_interval.
  side, fuse  (PiDiNet) pidinet_ref.side_ref / fuse_ref.
  tail        blur_f32, nms, blur_u8_bin: bit for bit against hed_ref.blur / nms_keep / blur_u8_bin.
  prep        bit for bit against oracle.image_prep.prepare_images, every replica; the scratch image against the oracle's first pass.
A planted error is a restatement of the kernel with one thing wrong (or a correct result with the part a wrong launch would leave
unwritten still at its poison); the host test holds each against the same check the GPU test applies."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

import helpers
import helper_forms as HF
import hed_ref as HR
import pidinet_forms as PF
import pidinet_ref as PR
from oracle import image_prep as O

F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8
DTYPES = (F32, F16, BF16)
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
POISON = helpers._POISON
U8_POISON = 0xA5
Case, pick, check = HF.Case, HF.pick, HF.check

# restated from csrc/hed.hip, csrc/pidinet.hip and csrc/imageprep.hip
THREADS = 256               # NT: every kernel below runs 256 threads per workgroup
QUAD = 4                    # stem and fuse: four neighbouring pixels of a row per thread
STEM_QUADS = THREADS // 8   # the stems: eight threads (8 output channels each) share a quad
BLUR_TILE = 64              # hed_blur_kernel: TS
TAPS_F32, TAPS_U8 = 25, 19  # kTapsF32, kTapsU8
R_F32, R_U8 = TAPS_F32 // 2, TAPS_U8 // 2
HED_STRIDES = (1, 2, 4, 8, 16)
PIDI_STRIDES = (1, 2, 4, 8)
PRECISION_BITS = 32 - 8 - 2


def pool_blocks(C):
    """2x2 pixel blocks per workgroup of hed_pool_proj_kernel<C / 8>"""
    return THREADS // (C // 8)


def groups(items, per):
    """(workgroups, items of the last one) of a launch of `items` work items, `per` to a workgroup"""
    n = -(-items // per)
    return n, items - (n - 1) * per


def ragged(items, per):
    return items % per != 0


# ---------------------------------------------------------------------------------------------------------------------------
# the stems
# ---------------------------------------------------------------------------------------------------------------------------
STEM_SIZES = ((1, 1, 4), (3, 3, 12), (2, 5, 68), (1, 130, 8), (2, 64, 64))          # (N, H, W)
STEM_SCALES = (1.0, 0.25)


def stem_frames(N, H, W):
    """uint8 [N, H, W, 3]: noise whose channels differ (red dark, blue bright: a swapped channel order moves every output), the corner
    pixels of every frame 255 and 0 (where a wrong padding shows)"""
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    fr = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.int64)
    fr[..., 0] = fr[..., 0] // 3
    fr[..., 2] = 255 - fr[..., 2] // 4
    fr[:, 0, 0] = 255
    fr[:, -1, -1] = 0
    return fr.to(U8).contiguous()


@functools.lru_cache(maxsize=None)
def _hed_sd():
    return HR.make_state_dict(21, "he")


@functools.lru_cache(maxsize=None)
def hed_stem_problem(N, H, W):
    """-> frames, w [64, 3, 3, 3], b [64], norm [3], scale, ref and mag fp64 [N, H, W, 64] (test_gpu_hed.py::test_stem's reference)"""
    sd = _hed_sd()
    w, b, norm = sd["block1.convs.0.weight"], sd["block1.convs.0.bias"], sd["norm"].reshape(3)
    scale = STEM_SCALES[STEM_SIZES.index((N, H, W)) % 2]
    frames = stem_frames(N, H, W)
    x = (frames.permute(0, 3, 1, 2).double() - norm.double().reshape(1, 3, 1, 1)) * scale
    pre = Fn.conv2d(x, w.double(), b.double() * scale, padding=1)
    mag = Fn.conv2d(x.abs(), w.double().abs(), (b.double() * scale).abs(), padding=1)
    return frames, w, b, norm, scale, pre.clamp_min(0).permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def hed_stem_share(got, ref, mag):
    """worst |got - ref| / bound of an fp16 [N, H, W, 64] result: 27 taps + the subtraction's rounding of every input"""
    return check(got, ref, helpers.igemm_bound(ref, mag, 28, 1.0, F16))


@functools.lru_cache(maxsize=None)
def pidi_stem_problem(N, H, W):
    """-> frames, the converted `cd` kernel [60, 3, 3, 3], ref and bound fp64 [N, 60, H, W] (pidinet_ref.stem_ref)"""
    frames = stem_frames(N, H, W)
    kern = PF.lib_convert("cd", PR.make_state_dict(21, "he")["init_block.weight"] * 4)
    ref, bound = PR.stem_ref(frames, kern)
    return frames, kern, ref, bound


def last_quad_at_poison(out_nhwc):
    """planted: the stem's last quad (the last four pixels of the last row of the last frame) never written"""
    o = out_nhwc.clone()
    o.reshape(-1, o.shape[-1])[-QUAD:] = POISON[F16]
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# HED pool + project
# ---------------------------------------------------------------------------------------------------------------------------
POOL_CS = (64, 128, 256, 512)
POOL_SHAPES = ((1, 2, 2), (1, 6, 10), (2, 10, 6), (3, 4, 4))          # 1, 15, 30 and 12 pixel blocks
POOL_INVS = (1.0, 4.0, 16.0)
POOL = [Case(id="pp-C%d-N%d-%dx%d-%s" % (C, N, H, W, "pool" if pooled else "proj"), C=C, N=N, H=H, W=W, pooled=pooled,
             inv=POOL_INVS[(i + j) % 3], blocks=N * (H // 2) * (W // 2))
        for i, C in enumerate(POOL_CS) for j, (N, H, W) in enumerate(POOL_SHAPES) for pooled in (True, False)]
POOL_BY_ID = {c.id: c for c in POOL}


@functools.lru_cache(maxsize=None)
def pool_problem(case_id):
    """-> h fp16 [N, H, W, C], wp [C], bp [1], ref and mag fp64 [N, H, W], the pooled map fp16 [N, H / 2, W / 2, C]"""
    c = POOL_BY_ID[case_id]
    g = HF._gen("pool", c.C, c.N, c.H, c.W)
    h = (torch.randn((c.N, c.H, c.W, c.C), generator=g) * 3).half()
    wp = torch.randn(c.C, generator=g) / c.C ** 0.5
    bp = torch.randn(1, generator=g)
    ref = (h.double() * wp.double()).sum(-1) * c.inv + bp.double()
    mag = (h.double().abs() * wp.double().abs()).sum(-1) * c.inv + bp.double().abs()
    pooled = Fn.max_pool2d(h.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).half().contiguous()
    return h, wp, bp, ref, mag, pooled


def pool_share(c, got, ref, mag):
    return check(got, ref, helpers.igemm_bound(ref, mag, c.C, 1.0, F32))


def pool_block_pixels(N, H, W):
    """flat pixel indices [blocks][4] of the 2x2 blocks in the kernel's order (q -> n, y2, x2)"""
    Hh, Wh = H // 2, W // 2
    q = torch.arange(N * Hh * Wh)
    n, rem = q // (Hh * Wh), q % (Hh * Wh)
    pix = (n * H + 2 * (rem // Wh)) * W + 2 * (rem % Wh)
    return torch.stack([pix, pix + 1, pix + W, pix + W + 1], 1)


def pool_last_group_at_poison(c, p, pooled):
    """planted: the last workgroup's pixel blocks never written -> (p, pooled)"""
    n, last = groups(c.blocks, pool_blocks(c.C))
    p, pooled = p.clone(), pooled.clone()
    p.reshape(-1)[pool_block_pixels(c.N, c.H, c.W)[c.blocks - last:].reshape(-1)] = POISON[F32]
    pooled.reshape(-1, c.C)[c.blocks - last:] = POISON[F16]
    return p, pooled


# ---------------------------------------------------------------------------------------------------------------------------
# HED fuse
# ---------------------------------------------------------------------------------------------------------------------------
FUSE_SIZES = ((1, 16, 16), (1, 16, 48), (1, 48, 16), (3, 80, 32), (2, 128, 64))          # (N, H, W)
FUSE_CHANNELS = (1, 3)


@functools.lru_cache(maxsize=None)
def hed_fuse_problem(N, H, W):
    """-> the five maps fp32 [N, H >> k, W >> k], ref, bound fp64 [N, H, W] (the mean logit; 16 * 2^-24 * mag) and numpy's bytes"""
    g = torch.Generator().manual_seed(H + W + N)
    maps = [torch.randn((N, H >> k, W >> k), generator=g) * 2 for k in range(5)]
    ref = np.stack([sum(HR.resize_linear(m[n].double().numpy(), H, W) for m in maps) / 5 for n in range(N)])
    mag = np.stack([sum(HR.resize_linear(m[n].double().abs().numpy(), H, W) for m in maps) / 5 for n in range(N)])
    want = np.stack([HR.fuse([m[n].numpy() for m in maps], H, W)[0] for n in range(N)])
    return maps, ref, 16 * 2.0 ** -24 * mag, want


def hed_fuse_check(got_u8, got_logit, ref, bound):
    """(worst logit |err| / bound, logits outside, bytes outside the interval the bound allows); got_u8 [N, H, W], one channel"""
    lg = np.asarray(got_logit, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        share = np.abs(lg - ref) / bound
    worst = float("inf") if not np.isfinite(lg).all() else float(share.max())
    return worst, HR.logit_failures(lg, ref, bound), HR.u8_failures(got_u8, ref, bound)


def lin_coords(dst, n, k, planted=None):
    """lin_coord of csrc/hed.hip for the output positions 0 .. dst - 1 on a map of n samples at stride 2^k, in fp32.
    planted: no_lower_clamp, align_corners"""
    d = np.arange(dst, dtype=np.float32)
    if planted == "align_corners":
        f = (d * np.float32((n - 1) / max(dst - 1, 1))).astype(np.float32)
    else:
        f = (d + np.float32(0.5)) * np.float32(1.0 / (1 << k)) - np.float32(0.5)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if planted != "no_lower_clamp":
        lo = s < 0
        s[lo], f[lo] = 0, 0
    hi = s >= n - 1
    s[hi], f[hi] = n - 1, 0
    return s, np.where(s + 1 < n, s + 1, n - 1), f


def hed_fuse_emulate(maps, H, W, planted=None):
    """hed_fuse_kernel in numpy fp32 (products and sums rounded one by one; the kernel may contract them) -> (uint8 [N, H, W], the logit).
    Reads go through the flat index the kernel forms, into the map between NaN (what lies in front of and behind it in the GPU test).
    planted: no_lower_clamp, align_corners, hw_swapped (lin_coord given the map's height for x and its width for y)"""
    N = maps[0].shape[0]
    one = np.float32(1)
    total = maps[0].numpy().astype(np.float32).copy()
    for k in range(1, 5):
        hk, wk = H >> k, W >> k
        nx, ny = (hk, wk) if planted == "hw_swapped" else (wk, hk)
        xa, xb, fx = lin_coords(W, nx, k, planted)
        ya, yb, fy = lin_coords(H, ny, k, planted)
        pad = (max(hk, wk) + 1) ** 2 + 2
        flat = np.concatenate([np.full(pad, np.nan, np.float32), maps[k].numpy().reshape(-1), np.full(pad, np.nan, np.float32)])
        base = pad + (np.arange(N) * hk * wk)[:, None, None]
        at = lambda y, x: flat[base + (y * wk)[None, :, None] + x[None, None, :]]
        with np.errstate(invalid="ignore"):
            r0 = at(ya, xa) * (one - fx) + at(ya, xb) * fx
            r1 = at(yb, xa) * (one - fx) + at(yb, xb) * fx
            total = total + (r0 * (one - fy)[None, :, None] + r1 * fy[None, :, None])
    mean = (total / np.float32(5)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (one / (one + np.exp(-mean))) * np.float32(255)
        u8 = np.nan_to_num(u, nan=0.0).clip(0, 255).astype(np.uint8)
    return u8, mean


# ---------------------------------------------------------------------------------------------------------------------------
# PiDiNet side + fuse (the cases of test_gpu_pidinet.py::test_side_and_fuse_forms)
# ---------------------------------------------------------------------------------------------------------------------------
PIDI_FUSE_SIZES = ((8, 8), (8, 24), (24, 8), (72, 40), (128, 64))          # (H, W), N = 2
PIDI_FUSE_N = 2


def pidi_fuse_planted(es, cw, cb, H, W, planted):
    """the fuse's logit [N, H, W] in fp64 with torch's bilinear.  planted: align_corners"""
    out = torch.zeros(es[0].shape[0], H, W, dtype=torch.float64) + float(cb)
    for e, w in zip(es, cw):
        out = out + float(w) * Fn.interpolate(e.double()[:, None], (H, W), mode="bilinear", align_corners=planted == "align_corners")[:, 0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# HED scribble tail
# ---------------------------------------------------------------------------------------------------------------------------
BLUR_SIZES = ((13, 13), (13, 64), (64, 13), (63, 65), (65, 63), (20, 77), (128, 64), (129, 130))
BLUR_U8_ONLY = ((10, 10),)
NMS_ONLY = ((1, 1), (1, 9), (9, 1), (2, 2))
TAIL_NS = (1, 3)
TAIL_NAMES = {1: (("waves",), ("plateaus",)), 3: (("isolated", "lines", "plateaus"), ("random", "lines", "waves"))}


def blur_tiles(H, W):
    """(tx, ty) of hed_blur_kernel's grid"""
    return -(-W // BLUR_TILE), -(-H // BLUR_TILE)


def tail_stack(N, H, W):
    """uint8 [N, H, W] of hed_ref.tail_maps, the maps of TAIL_NAMES by the size's place in its table (a dense random map alone sets every
    byte of the binarised blur, so it goes with two sparse ones); maps with a side of 1, which tail_maps cannot draw: noise above and
    below nms' threshold"""
    if min(H, W) < 2:
        rng = np.random.RandomState(H * 100 + W + N)
        return (rng.rand(N, H, W) * 255).astype(np.uint8) | np.uint8(128 if H * W == 1 else 0)
    maps = HR.tail_maps(H, W)
    sizes = BLUR_SIZES + BLUR_U8_ONLY + NMS_ONLY
    return np.stack([maps[k] for k in TAIL_NAMES[N][sizes.index((H, W)) % 2]])


@functools.lru_cache(maxsize=None)
def tail_reference(N, H, W):
    """the stages as test_gpu_hed.py::test_tail_stages_are_exact chains them -> dict: stack uint8 [N]; where H, W > 12: blur fp32 [N],
    nms_in fp32 [2 N] (the raw maps as floats, then the blurred ones) else the raw maps alone; nms uint8; where H, W > 9: bin_in uint8
    (the thinned maps, then the raw ones) and bin uint8"""
    stack = tail_stack(N, H, W)
    out = {"stack": stack}
    nms_in = stack.astype(np.float32)
    if min(H, W) > R_F32:
        taps = HR.gaussian_taps(TAPS_F32)
        out["blur"] = np.stack([HR.blur(m.astype(np.float32), taps) for m in stack])
        nms_in = np.concatenate([nms_in, out["blur"]])
    out["nms_in"] = nms_in
    out["nms"] = np.stack([HR.nms_keep(x) for x in nms_in])
    if min(H, W) > R_U8:
        out["bin_in"] = np.concatenate([out["nms"], stack])
        out["bin"] = np.stack([HR.blur_u8_bin(u) for u in out["bin_in"]])
    return out


def blur_planted(x, taps, planted):
    """hed_ref.blur of one fp32 map with one thing wrong: clamp (the border replicated instead of reflected), cols_first (the column
    pass before the row pass)"""
    r = len(taps) // 2
    H, W = x.shape
    p = np.pad(x, r, mode="edge" if planted == "clamp" else "reflect")
    if planted == "cols_first":
        p = p.T
        H, W = W, H
    acc = p[:, 0:W] * taps[0]
    for t in range(1, len(taps)):
        acc = acc + p[:, t:t + W] * taps[t]
    acc2 = acc[0:H] * taps[0]
    for t in range(1, len(taps)):
        acc2 = acc2 + acc[t:t + H] * taps[t]
    return acc2.T.copy() if planted == "cols_first" else acc2


def blur_tile_row_mod(want, fill):
    """planted: the tile row decoded as tr % tx instead of tr / tx -> what the launch leaves of a correct result [N, H, W]: every tile
    writes the place its wrong origin names, the rest stays at `fill`"""
    N, H, W = want.shape
    tx, ty = blur_tiles(H, W)
    out = np.full_like(want, fill)
    for tr in range(tx * ty):
        y0, x0 = (tr % tx) * BLUR_TILE, (tr % tx) * BLUR_TILE
        out[:, y0:y0 + BLUR_TILE, x0:x0 + BLUR_TILE] = want[:, y0:y0 + BLUR_TILE, x0:x0 + BLUR_TILE]
    return out


def nms_across_the_seam(x):
    """planted: hed_nms_kernel without its frame arithmetic: the stack [N, H, W] thinned as ONE map of N H rows"""
    N, H, W = x.shape
    return HR.nms_keep(x.reshape(N * H, W)).reshape(N, H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# image preparation
# ---------------------------------------------------------------------------------------------------------------------------
PREP_SIZES = {                                         # (Hin, Win, H, W)
    "h": ((64, 72, 64, 64), (64, 40, 64, 64)),
    "v": ((72, 64, 64, 64), (40, 64, 64, 64)),
    "both": ((17, 33, 24, 40), (255, 257, 256, 256), (9, 8, 8, 16)),
    "neither": ((24, 40, 24, 40),),
    "ksize": ((8, 2048, 8, 8), (2048, 8, 8, 8)),
    "one": ((1, 1, 8, 8), (1, 300, 8, 8)),
}
PREP_FS, PREP_REPS, PREP_CFGS = (1, 3), (1, 2, 3), (1, 2)
PREP = []
for _kind, _sizes in PREP_SIZES.items():
    for _s, (_hi, _wi, _h, _w) in enumerate(_sizes):
        for _j in range(3):
            _i = len(PREP)
            _F, _rep, _cfg, _dt = PREP_FS[(_i + _i // 6) % 2], PREP_REPS[(_i + _i // 3) % 3], PREP_CFGS[(_i // 2 + _i // 6) % 2], DTYPES[_j]
            if (_hi, _wi) == (255, 257) and _F * _rep * _cfg > 6:          # the largest output of the table stays at 6 x 3 x 256 x 256
                _rep = 1
            PREP.append(Case(id="prep-%dx%d-%dx%d-F%d-rep%d-cfg%d-%s" % (_hi, _wi, _h, _w, _F, _rep, _cfg, DT_NAME[_dt]), kind=_kind, Hin=_hi,
                             Win=_wi, H=_h, W=_w, F=_F, rep=_rep, cfg=_cfg, dt=_dt))
PREP_BY_ID = {c.id: c for c in PREP}


def prep_items(c):
    """work items of the two launches: (horizontal pass or 0, vertical pass + store)"""
    return (c.F * c.Hin * c.W if c.Win != c.W else 0), c.F * c.H * c.W


def rand_img(h, w, seed):
    """tests/test_image_prep.py::_rand_img (restated: that module needs Pillow to import; the host test holds the two together)"""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    base[: h // 3, : w // 2] = 255
    base[h // 2:, w // 2:] = 0
    return base


@functools.lru_cache(maxsize=None)
def prep_frames(Hin, Win, F):
    """F distinct uint8 frames [Hin, Win, 3]: _rand_img + 0 / 255 stripes of period 2 .. 6 along x (a band of rows) and along y (a band of
    columns): the Lanczos lobes overshoot on them, so clip8 clamps at both ends in whichever pass meets them; a one-pixel frame holds a
    0 and a 255 among its channels"""
    out = []
    for f in range(F):
        img = rand_img(Hin, Win, 7 * f + Hin * 1000 + Win)
        p = 2 + (f + Hin + Win) % 5
        sx = np.where(np.arange(Win) % p < (p + 1) // 2, 255, 0).astype(np.uint8)
        sy = np.where(np.arange(Hin) % p < (p + 1) // 2, 255, 0).astype(np.uint8)
        img[Hin // 3:max(Hin // 2, Hin // 3 + 1)] = sx[None, :, None]
        img[Hin // 2:, :Win // 2] = sy[Hin // 2:, None, None]
        if Hin * Win == 1:
            img[0, 0] = (0, 255, 77 + f)
        elif Hin == 1:
            img[0, :, 1] = 255 - img[0, :, 0]
        out.append(img)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def prep_resized(Hin, Win, H, W, F):
    """the oracle's resize of the frames: (after the horizontal pass uint8 [F, Hin, W, 3], the result uint8 [F, H, W, 3])"""
    fr = prep_frames(Hin, Win, F)
    mid = [O._resample_axis(f, W, 1) if Win != W else f for f in fr]
    return np.stack(mid), np.stack([O._resample_axis(m, H, 0) if Hin != H else m for m in mid])


def prep_expected(c):
    """oracle.image_prep.prepare_images of the case -> [cfg, rep F, 3, H, W] in the case's dtype"""
    return O.prepare_images(list(prep_frames(c.Hin, c.Win, c.F)), c.W, c.H, c.rep, 1, dtype=c.dt, do_classifier_free_guidance=c.cfg == 2)


def prep_tables(c):
    """(hks, hbounds, hk, vks, vbounds, vk) as ctrl_adapter_amd.image_prep builds them; None for an axis that is not resampled"""
    from ctrl_adapter_amd.image_prep import _coeffs
    h = _coeffs(c.Win, c.W) if c.Win != c.W else (0, None, None)
    v = _coeffs(c.Hin, c.H) if c.Hin != c.H else (0, None, None)
    return h + v


def _prep_pass(src, axis, table, planted, wrap):
    """one pass of csrc/imageprep.hip over `axis` of uint8 [F, H, W, 3] with the flat weight table the kernel indexes"""
    ks, bounds, kk = table
    flat = np.concatenate([kk.reshape(-1).astype(np.int64), np.zeros(ks, np.int64)])
    stride = ks - 1 if planted == "kk_stride" else ks
    s = np.moveaxis(src, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + s.shape[1:], np.uint8)
    for o in range(bounds.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(s.shape[1:], 0 if planted == "no_round" else 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += s[lo + x] * flat[o * stride + x]
        acc >>= PRECISION_BITS
        out[o] = (acc & 255 if wrap else acc.clip(0, 255)).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def prep_emulate(c, planted=None):
    """the two kernels restated in integers -> [cfg, rep F, 3, H, W] in the case's dtype.  planted: no_h_clamp (the horizontal pass
    stores the low byte of its sum), vertical_first, no_round (the 1 << 21 missing), mul_inv255 (v * (1 / 255f)), replica_index
    (frame f rep + r), kk_stride (ksize - 1 between the rows of the weight table), cfg_missing (the second copy left at its poison)"""
    from ctrl_adapter_amd.image_prep import _coeffs
    x = np.stack(prep_frames(c.Hin, c.Win, c.F))
    passes = [(2, c.Win, c.W), (1, c.Hin, c.H)]
    if planted == "vertical_first":
        passes.reverse()
    for axis, n_in, n_out in passes:
        if n_in != n_out:
            x = _prep_pass(x, axis, _coeffs(n_in, n_out), planted, wrap=planted == "no_h_clamp" and axis == 2)
    v = torch.from_numpy(x.astype(np.float32))
    val = v * torch.tensor(1.0 / 255.0, dtype=F32) if planted == "mul_inv255" else v / 255.0
    val = val.permute(0, 3, 1, 2).to(c.dt)                                   # [F, 3, H, W]
    out = torch.full((c.cfg, c.rep * c.F, 3, c.H, c.W), POISON[c.dt], dtype=c.dt)
    for g in range(c.cfg if planted != "cfg_missing" else 1):
        for r in range(c.rep):
            for f in range(c.F):
                out[g, (f * c.rep + r) if planted == "replica_index" else (r * c.F + f)] = val[f]
    return out


def prep_differs(got, want):
    """number of elements whose bits differ"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((helpers._bits(got) != helpers._bits(want)).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(ptr, odd_ptr):
    """[(name, symbol, ctypes argument list without the stream, part of the message)]: `ptr` any 16-byte aligned address the call may
    name (a refused call dereferences nothing), `odd_ptr` one that is 2 mod 16.  The stream goes last on every entry point."""
    import ctypes as C
    P, I, F = (lambda: C.c_void_p(ptr)), C.c_int, C.c_float
    null, odd = C.c_void_p(0), C.c_void_p(odd_ptr)
    n3 = (C.c_float * 3)(1.0, 2.0, 3.0)
    f5, f37 = (C.c_float * 5)(), (C.c_float * 37)()
    m5, m4 = (C.c_void_p * 5)(*[ptr] * 5), (C.c_void_p * 4)(*[ptr] * 4)
    hst = lambda W=8, H=2: [P(), I(1), I(H), I(W), P(), P(), n3, F(1.0), P(), null]
    pst = lambda W=8, out=None: [P(), I(1), I(2), I(W), P(), out or P(), null]
    pp = lambda H=2, W=2, Cc=64: [P(), I(1), I(H), I(W), I(Cc), P(), P(), F(1.0), null, P()]
    hf = lambda H=16, W=16, ch=1, out=None: [m5, I(1), I(H), I(W), I(ch), out or P(), null]
    pf = lambda H=8, W=8, out=None: [m4, I(1), I(H), I(W), f5, I(0), I(1), out or P(), null]
    prep = lambda Hin=8, Win=16, hb=True, vb=False, tmp=True, cfg=1, hks=19: [
        P(), I(1), I(Hin), I(Win), P() if hb else null, P() if hb else null, I(hks if hb else 0), P() if vb else null, P() if vb else null,
        I(19 if vb else 0), P() if tmp else null, P(), I(0), I(8), I(8), I(1), I(cfg)]
    return [
        ("hed stem W % 4", "ctrl_op_hed_stem", hst(W=6), "hed_stem: W must be a multiple of 4"),
        ("hed stem H = 0", "ctrl_op_hed_stem", hst(H=0), "hed_stem: N, H and W must be positive"),
        ("pidi stem W % 4", "ctrl_op_pidi_stem", pst(W=6), "pidi_stem: W must be a multiple of 4"),
        ("pidi stem misaligned out", "ctrl_op_pidi_stem", pst(out=odd), "pidi_stem: w and out must be 16-byte aligned"),
        ("pool_proj odd H", "ctrl_op_hed_pool_proj", pp(H=3), "hed_pool_proj: H and W must be even"),
        ("pool_proj odd W", "ctrl_op_hed_pool_proj", pp(W=5), "hed_pool_proj: H and W must be even"),
        ("pool_proj C = 96", "ctrl_op_hed_pool_proj", pp(Cc=96), "hed_pool_proj: C must be 64, 128, 256 or 512"),
        ("hed fuse H % 16", "ctrl_op_hed_fuse", hf(H=24), "hed_fuse: H and W must be multiples of 16"),
        ("hed fuse W % 16", "ctrl_op_hed_fuse", hf(W=8), "hed_fuse: H and W must be multiples of 16"),
        ("hed fuse misaligned out", "ctrl_op_hed_fuse", hf(out=odd), "hed_fuse: out must be 4-byte aligned"),
        ("hed fuse 2 channels", "ctrl_op_hed_fuse", hf(ch=2), "hed_fuse: out_channels must be 1 or 3"),
        ("pidi fuse H % 8", "ctrl_op_pidi_fuse", pf(H=12), "pidi_fuse: H and W must be multiples of 8"),
        ("pidi fuse misaligned out", "ctrl_op_pidi_fuse", pf(out=odd), "pidi_fuse: out must be 4-byte aligned"),
        ("pidi side misaligned a4", "ctrl_op_pidi_side", [odd, P(), I(1), I(8), I(8), f37, P()], "pidi_side: a4 must be 16-byte aligned"),
        ("blur_f32 H <= radius", "ctrl_op_hed_blur_f32", [P(), I(1), I(R_F32), I(64), P()], "hed_blur_f32: H and W must exceed the blur radius"),
        ("blur_f32 W <= radius", "ctrl_op_hed_blur_f32", [P(), I(1), I(64), I(R_F32), P()], "hed_blur_f32: H and W must exceed the blur radius"),
        ("blur_u8_bin H <= radius", "ctrl_op_hed_blur_u8_bin", [P(), I(1), I(R_U8), I(64), I(1), P()],
         "hed_blur_u8_bin: H and W must exceed the blur radius"),
        ("blur_u8_bin 2 channels", "ctrl_op_hed_blur_u8_bin", [P(), I(1), I(64), I(64), I(2), P()], "hed_blur_u8_bin: out_channels must be 1 or 3"),
        ("nms N = 0", "ctrl_op_hed_nms", [P(), I(0), I(8), I(8), P()], "hed_nms: N, H and W must be positive"),
        ("prep tables for an axis that is not resampled", "ctrl_prepare_images", prep(Win=8), "prepare_images: weight tables must be given exactly"),
        ("prep vertical tables for an axis that is not resampled", "ctrl_prepare_images", prep(vb=True), "prepare_images: weight tables must be given exactly"),
        ("prep no tables for a resampled width", "ctrl_prepare_images", prep(hb=False), "prepare_images: weight tables must be given exactly"),
        ("prep no tables for a resampled height", "ctrl_prepare_images", prep(Hin=9), "prepare_images: weight tables must be given exactly"),
        ("prep cfg = 3", "ctrl_prepare_images", prep(cfg=3), "prepare_images: bad argument"),
        ("prep null tmp", "ctrl_prepare_images", prep(tmp=False), "prepare_images: horizontal pass needs a scratch image"),
        ("prep ksize 0", "ctrl_prepare_images", prep(hks=0), "prepare_images: horizontal pass needs a scratch image"),
    ]
