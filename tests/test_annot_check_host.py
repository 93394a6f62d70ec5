"""Self-test of the annotator and image-preparation checks (tests/annot_forms.py), no GPU: the tables hold the edges they declare (asserted
from constants restated from csrc/hed.hip, csrc/pidinet.hip and csrc/imageprep.hip), no exact case passes vacuously, the restated kernels
agree with the references the GPU tests compare with, every planted error is rejected by the same check on a named case, the entry points
refuse what they must before any launch, and the oracle's resize is Pillow's at every size of the preparation table."""
import ctypes

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import annot_forms as A
import hed_ref as HR
import pidinet_forms as PF
import pidinet_ref as PR
from oracle import image_prep as O

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# the tables hold the declared edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    assert (A.THREADS, A.QUAD, A.STEM_QUADS, A.BLUR_TILE, A.R_F32, A.R_U8) == (256, 4, 32, 64, 12, 9)
    assert [A.pool_blocks(C) for C in A.POOL_CS] == [32, 16, 8, 4]
    assert (A.TAPS_F32, A.TAPS_U8) == (HR.auto_ksize(3.0, False), HR.auto_ksize(3.0, True))
    assert A.HED_STRIDES == tuple(1 << k for k in range(5)) and A.PIDI_STRIDES == tuple(1 << k for k in range(4))
    assert A.PRECISION_BITS == O.PRECISION_BITS == 22


def test_stem_table_holds_the_declared_edges():
    quads = {s: s[0] * s[1] * s[2] // A.QUAD for s in A.STEM_SIZES}
    assert all(W % A.QUAD == 0 for _, _, W in A.STEM_SIZES)
    assert quads[(1, 1, 4)] == 1 and any(W // A.QUAD == 1 for _, _, W in A.STEM_SIZES)                       # wq = 1: every quad meets both borders
    assert any(H < 3 for _, H, _ in A.STEM_SIZES) and any(H > 2 * A.BLUR_TILE and H > 8 * W for _, H, W in A.STEM_SIZES)          # H < 3; a tall frame
    tails = {s: A.groups(q, A.STEM_QUADS) for s, q in quads.items()}
    assert any(n > 1 and last < A.STEM_QUADS for n, last in tails.values())                                  # the q >= quads exit behind full workgroups
    assert any(n == 1 and last < A.STEM_QUADS for n, last in tails.values()) and any(last == A.STEM_QUADS for _, last in tails.values())
    assert sum(A.ragged(q, A.STEM_QUADS) for q in quads.values()) == 4
    assert any(N > 1 and (H * W // A.QUAD) % A.STEM_QUADS for N, H, W in A.STEM_SIZES)                         # a workgroup over two frames
    for N, H, W in A.STEM_SIZES:
        fr = A.stem_frames(N, H, W)
        assert fr.shape == (N, H, W, 3) and bool((fr[:, 0, 0] == 255).all()) and bool((fr[:, -1, -1] == 0).all())
        assert float(fr[..., 0].float().mean()) + 60 < float(fr[..., 2].float().mean())                       # red dark, blue bright
    assert {A.hed_stem_problem(*s)[4] for s in A.STEM_SIZES} == set(A.STEM_SCALES)


def test_pool_table_holds_the_declared_edges():
    assert {(c.C, c.N, c.H, c.W, c.pooled) for c in A.POOL} == {(C, N, H, W, p) for C in (64, 128, 256, 512)
                                                                for (N, H, W) in ((1, 2, 2), (1, 6, 10), (2, 10, 6), (3, 4, 4)) for p in (True, False)}
    assert {c.blocks for c in A.POOL} == {1, 15, 30, 12} and len({c.id for c in A.POOL}) == len(A.POOL)
    for C in A.POOL_CS:
        per = A.pool_blocks(C)
        assert A.ragged(15, per) and A.ragged(30, per)                                  # a ragged last workgroup for every L
        t = [c for c in A.POOL if c.C == C]
        behind_full = any(A.groups(c.blocks, per)[0] > 1 and A.ragged(c.blocks, per) for c in t)
        assert behind_full == (per <= 30)                                               # (C = 64 takes 32 blocks: its largest case is one workgroup)
        assert any(c.blocks < per for c in t) and {c.pooled for c in t if c.blocks in (15, 30)} == {True, False}
    assert any(not A.ragged(c.blocks, A.pool_blocks(c.C)) for c in A.POOL) and any(c.N > 1 and c.H > c.W for c in A.POOL)
    assert {c.inv for c in A.POOL} == set(A.POOL_INVS)
    c = A.pick(A.POOL, C=128, N=2, H=10, W=6)                                           # the restated index arithmetic is the 2x2 pooling
    h, _, _, _, _, pooled = A.pool_problem(c.id)
    px = A.pool_block_pixels(c.N, c.H, c.W)
    assert torch.equal(h.reshape(-1, c.C)[px].float().amax(1).half(), pooled.reshape(-1, c.C))
    assert sorted(px.reshape(-1).tolist()) == list(range(c.N * c.H * c.W))


def test_fuse_tables_hold_the_declared_edges():
    deepest = {(H >> 4, W >> 4) for _, H, W in A.FUSE_SIZES}
    assert {(1, 1), (1, 3), (3, 1)} <= deepest and all(H % 16 == 0 and W % 16 == 0 for _, H, W in A.FUSE_SIZES)
    assert any(H > W for _, H, W in A.FUSE_SIZES) and any(H < W for _, H, W in A.FUSE_SIZES)
    quads = [N * H * W // A.QUAD for N, H, W in A.FUSE_SIZES]
    assert any(q > A.THREADS and A.ragged(q, A.THREADS) for q in quads) and any(q < A.THREADS for q in quads)
    assert any(not A.ragged(q, A.THREADS) for q in quads) and any(N == 3 for N, _, _ in A.FUSE_SIZES)
    # lin_coord's two clamps are both taken, and on the 1 x 1 map both at once
    for n, k in ((1, 4), (3, 4), (5, 4)):
        s, s1, f = A.lin_coords(n << k, n, k)
        raw = (np.arange(n << k) + 0.5) / (1 << k) - 0.5
        assert (raw < 0).any() and (np.floor(raw) >= n - 1).any() and s.min() == 0 and s1.max() == n - 1 and (f[raw < 0] == 0).all()
    for dst, n, k in ((16, 1, 4), (48, 3, 4), (80, 5, 4), (64, 32, 1)):                  # the restatement is hed_ref's (cv2's) coordinates
        a, b = A.lin_coords(dst, n, k), HR._lin_coords(dst, n, False)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # PiDiNet: the side kernel at every stride, the fuse in quads
    assert all(H % 8 == 0 and W % 8 == 0 for H, W in A.PIDI_FUSE_SIZES) and {(H >> 3, W >> 3) for H, W in A.PIDI_FUSE_SIZES} >= {(1, 1), (1, 3), (3, 1)}
    side = [A.PIDI_FUSE_N * (H >> k) * (W >> k) for H, W in A.PIDI_FUSE_SIZES for k in range(4)]
    assert any(t > A.THREADS and A.ragged(t, A.THREADS) for t in side) and any(t < A.THREADS for t in side) and any(not A.ragged(t, A.THREADS) for t in side)
    pq = [A.PIDI_FUSE_N * H * W // A.QUAD for H, W in A.PIDI_FUSE_SIZES]
    assert any(q > A.THREADS and A.ragged(q, A.THREADS) for q in pq) and any(not A.ragged(q, A.THREADS) for q in pq)
    assert any(H > W for H, W in A.PIDI_FUSE_SIZES) and (128, 64) in PF.FUSE_SIZES and PF.DETECTOR_CASES["128x64"] == (2, 128, 64)


def test_tail_tables_hold_the_declared_edges():
    T = A.BLUR_TILE
    tiles = {s: A.blur_tiles(*s) for s in A.BLUR_SIZES}
    assert any(ty > 1 and tx == 1 for tx, ty in tiles.values()) and any(tx > 1 and ty == 1 for tx, ty in tiles.values())          # tr / tx against tr % tx
    assert any(tx > 1 and ty > 1 for tx, ty in tiles.values())
    assert any(H > T and H % T for H, _ in A.BLUR_SIZES) and any(W > T and W % T for _, W in A.BLUR_SIZES)                        # a partial tile behind a full one
    assert any(H % T == 0 and W % T == 0 for H, W in A.BLUR_SIZES)
    assert any(W == A.R_F32 + 1 for _, W in A.BLUR_SIZES) and any(H == A.R_F32 + 1 for H, _ in A.BLUR_SIZES)                      # the smallest map the op takes
    assert any(W < T and W % 4 for _, W in A.BLUR_SIZES) and any(W > T and W % 4 for _, W in A.BLUR_SIZES)                        # both reflections in one tile
    assert all(min(s) == A.R_U8 + 1 for s in A.BLUR_U8_ONLY) and all(min(s) > A.R_F32 for s in A.BLUR_SIZES)
    assert {(1, 1), (1, 9), (9, 1), (2, 2)} == set(A.NMS_ONLY)
    totals = [N * H * W * 2 for N in A.TAIL_NS for H, W in A.BLUR_SIZES] + [N * H * W for N in A.TAIL_NS for H, W in A.NMS_ONLY + A.BLUR_U8_ONLY]
    assert any(t > A.THREADS and A.ragged(t, A.THREADS) for t in totals) and any(t < A.THREADS for t in totals) and any(not A.ragged(t, A.THREADS) for t in totals)
    names = set()
    for N in A.TAIL_NS:
        for i, (H, W) in enumerate(A.BLUR_SIZES + A.BLUR_U8_ONLY + A.NMS_ONLY):
            ref = A.tail_reference(N, H, W)
            assert ref["stack"].shape == (N, H, W) and int((ref["nms"] > 0).sum()) > 0, (N, H, W)          # nothing passes vacuously
            if min(H, W) >= 2:
                names |= set(A.TAIL_NAMES[N][i % 2])
            if (H, W) in A.BLUR_SIZES:
                assert int((ref["nms"][:N] > 0).sum()) > 0 and int((ref["nms"][N:] > 0).sum()) > 0, (N, H, W)
                assert ref["blur"].dtype == np.float32 and float(ref["blur"].max()) > 127.0
            if "bin" in ref:
                n_set = int((ref["bin"] > 0).sum())
                assert n_set > 0, (N, H, W)
                assert n_set < ref["bin"].size or max(H, W) < A.BLUR_TILE, (N, H, W)          # (a 13 x 13 map under a 19-tap blur can be all set)
    assert names == set(HR.tail_maps(16, 16))


def test_prep_table_holds_the_declared_edges():
    sizes = [(c.Hin, c.Win, c.H, c.W) for c in A.PREP]
    assert set(sizes) == {(64, 72, 64, 64), (64, 40, 64, 64), (72, 64, 64, 64), (40, 64, 64, 64), (17, 33, 24, 40), (255, 257, 256, 256), (9, 8, 8, 16),
                          (24, 40, 24, 40), (8, 2048, 8, 8), (2048, 8, 8, 8), (1, 1, 8, 8), (1, 300, 8, 8)}
    assert len({c.id for c in A.PREP}) == len(A.PREP)
    for c in A.PREP:          # the kinds are what they say
        assert (c.Win != c.W, c.Hin != c.H) == {"h": (True, False), "v": (False, True), "both": (True, True), "neither": (False, False),
                                                 "ksize": (c.Win != c.W, c.Hin != c.H), "one": (True, True)}[c.kind], c.id
        assert not (c.Win != c.W and c.Hin != c.H and c.Hin > 32 * c.Win), c.id          # Pillow's pass order on tall slivers
    assert any(c.Win > c.W for c in A.PREP if c.kind == "h") and any(c.Win < c.W for c in A.PREP if c.kind == "h")
    assert any(c.Hin > c.H for c in A.PREP if c.kind == "v") and any(c.Hin < c.H for c in A.PREP if c.kind == "v")
    assert {A.prep_tables(c)[0] for c in A.PREP if c.Win == 2048} == {1537} and {A.prep_tables(c)[3] for c in A.PREP if c.Hin == 2048} == {1537}
    # the ragged tail and the exact fit of both kernels, and every value of every lever at both
    hi = lambda n: n > A.THREADS and A.ragged(n, A.THREADS)
    ex = lambda n: n >= A.THREADS and not A.ragged(n, A.THREADS)
    assert any(hi(A.prep_items(c)[0]) for c in A.PREP) and any(ex(A.prep_items(c)[0]) for c in A.PREP) and any(0 < A.prep_items(c)[0] < A.THREADS for c in A.PREP)
    for lever, values in (("F", A.PREP_FS), ("rep", A.PREP_REPS), ("cfg", A.PREP_CFGS), ("dt", A.DTYPES)):
        for v in values:
            assert any(hi(A.prep_items(c)[1]) for c in A.PREP if c[lever] == v), (lever, v, "ragged")
            assert any(ex(A.prep_items(c)[1]) for c in A.PREP if c[lever] == v), (lever, v, "exact")
    assert {(c.F, c.rep, c.cfg) for c in A.PREP} >= {(3, 3, 2), (3, 2, 2), (1, 1, 1)} and max(c.cfg * c.rep * c.F * 3 * c.H * c.W for c in A.PREP) <= 6 * 3 * 256 * 256
    for c in A.PREP:
        want = A.prep_expected(c)
        assert want.shape == (c.cfg, c.rep * c.F, 3, c.H, c.W) and want.dtype == c.dt
        assert float(want.min()) == 0.0 and float(want.max()) == 1.0, c.id          # the oracle's output holds both 0 and 255
        fr = A.prep_frames(c.Hin, c.Win, c.F)
        assert len({f.tobytes() for f in fr}) == c.F
    img = A.rand_img(40, 64, 5)
    assert img.shape == (40, 64, 3) and img.dtype == np.uint8 and bool((img[:13, :32] == 255).all()) and bool((img[20:, 32:] == 0).all())


def test_prep_clip8_clamps_at_both_ends_in_both_passes():
    """on the sizes that resample both axes the sums leave 0 .. 255 at both ends before clip8, in the horizontal pass and in the vertical"""
    from ctrl_adapter_amd.image_prep import _coeffs
    for Hin, Win, H, W in A.PREP_SIZES["both"]:
        x = np.stack(A.prep_frames(Hin, Win, 3)).astype(np.int64)
        for axis, n_in, n_out in ((2, Win, W), (1, Hin, H)):
            ks, bounds, kk = _coeffs(n_in, n_out)
            s = np.moveaxis(x, axis, 0)
            lo = hi = False
            out = []
            for o in range(n_out):
                acc = sum(s[bounds[o, 0] + t] * int(kk[o, t]) for t in range(bounds[o, 1])) + (1 << 21)
                lo, hi = lo or bool((acc < 0).any()), hi or bool(((acc >> 22) > 255).any())
                out.append((acc >> 22).clip(0, 255))
            assert lo and hi, (Hin, Win, H, W, axis)
            x = np.moveaxis(np.stack(out), 0, axis)


def test_rand_img_is_test_image_preps():
    pytest.importorskip("PIL.Image")
    import test_image_prep as TP
    for h, w, s in ((64, 72, 3), (1, 1, 0), (9, 8, 11)):
        assert np.array_equal(A.rand_img(h, w, s), TP._rand_img(h, w, s))


# ---------------------------------------------------------------------------------------------------------------------------
# the restated kernels agree with the references
# ---------------------------------------------------------------------------------------------------------------------------
def test_emulations_pass_the_checks():
    worst = 0.0
    for N, H, W in A.FUSE_SIZES:
        maps, ref, bound, want = A.hed_fuse_problem(N, H, W)
        u8, lg = A.hed_fuse_emulate(maps, H, W)
        share, nl, nu = A.hed_fuse_check(u8, lg, ref, bound)
        worst = max(worst, share)
        assert nl == 0 and nu == 0 and share <= 1.0, (N, H, W, share)
        assert int((u8 != want).sum()) <= u8.size // 100                                # numpy's own bytes, up to a truncation at an integer
    print("ANNOT-HOST hed fuse: worst emulation / bound %.3f" % worst)
    for c in A.PREP:
        assert A.prep_differs(A.prep_emulate(c), A.prep_expected(c)) == 0, c.id
    for Hin, Win, H, W in {(c.Hin, c.Win, c.H, c.W) for c in A.PREP}:                    # the first pass is the oracle's
        mid, out = A.prep_resized(Hin, Win, H, W, 1)
        assert np.array_equal(out[0], O.pil_resize_lanczos(A.prep_frames(Hin, Win, 1)[0], W, H)) and mid.shape == (1, Hin, W, 3)
    x = A.tail_reference(1, 20, 77)["stack"][0].astype(np.float32)
    for taps in (HR.gaussian_taps(A.TAPS_F32), HR.gaussian_taps(A.TAPS_U8)):
        assert np.array_equal(A.blur_planted(x, taps, None), HR.blur(x, taps))


# ---------------------------------------------------------------------------------------------------------------------------
# every planted error is rejected on a named case
# ---------------------------------------------------------------------------------------------------------------------------
def test_planted_errors_are_rejected_hed_and_pidinet():
    # the stems: the last quad left at its poison; the channel order
    for size in ((2, 5, 68), (1, 1, 4), (1, 130, 8)):
        _, _, _, _, _, ref, mag = A.hed_stem_problem(*size)
        good = ref.half()
        assert A.hed_stem_share(good, ref, mag) <= 1.0 and A.hed_stem_share(A.last_quad_at_poison(good), ref, mag) > 1.0, size
    for size in ((3, 3, 12), (1, 1, 4)):
        frames, kern, ref, bound = A.pidi_stem_problem(*size)
        good = ref.half()
        left = A.last_quad_at_poison(good.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
        assert A.check(good, ref, bound) <= 1.0 and A.check(left, ref, bound) > 1.0, size
        swapped = PR.stem_ref(frames.flip(-1), kern)[0]                                 # RGB where the net takes BGR
        assert int(((swapped - ref).abs() > bound).sum()) > ref.numel() // 2, size
    # pool + project: the last workgroup left at its poison
    for c in (A.pick(A.POOL, C=512, blocks=15, pooled=True), A.pick(A.POOL, C=64, blocks=30, pooled=True), A.pick(A.POOL, C=256, blocks=1, pooled=True)):
        _, _, _, ref, mag, pooled = A.pool_problem(c.id)
        good = ref.float()
        p, pl = A.pool_last_group_at_poison(c, good, pooled)
        assert A.pool_share(c, good, ref, mag) <= 1.0 and A.pool_share(c, p, ref, mag) > 1.0 and not torch.equal(pl, pooled), c.id
        n, last = A.groups(c.blocks, A.pool_blocks(c.C))
        assert int((p != good).sum()) == 4 * last and int((pl != pooled).any(-1).sum()) == last
    # fuse: lin_coord
    for size, planted in (((1, 16, 16), "no_lower_clamp"), ((3, 80, 32), "no_lower_clamp"), ((1, 16, 48), "hw_swapped"), ((1, 48, 16), "hw_swapped"),
                          ((3, 80, 32), "hw_swapped"), ((3, 80, 32), "align_corners"), ((1, 16, 16), "align_corners"), ((2, 128, 64), "align_corners")):
        maps, ref, bound, _ = A.hed_fuse_problem(*size)
        share, nl, nu = A.hed_fuse_check(*A.hed_fuse_emulate(maps, size[1], size[2], planted), ref, bound)
        assert share > 1.0 and nl > 0, (size, planted)
    g = torch.Generator().manual_seed(5)
    for H, W in ((8, 24), (72, 40)):
        es = [torch.randn((2, H >> k, W >> k), generator=g) for k in range(4)]
        cw, cb = [0.6, -0.5, 0.4, 0.5], 0.1
        ref, bound = PR.fuse_ref(es, cw, cb, H, W)
        assert A.check(A.pidi_fuse_planted(es, cw, cb, H, W, None), ref, bound) <= 1.0
        assert A.check(A.pidi_fuse_planted(es, cw, cb, H, W, "align_corners"), ref, bound) > 1.0, (H, W)
    # the tail: exact, so one differing value rejects
    f32p, u8p = float(A.POISON[F32]), A.U8_POISON
    for (N, H, W), key, fill in (((1, 128, 64), "blur", f32p), ((3, 65, 63), "blur", f32p), ((1, 129, 130), "bin", u8p), ((3, 128, 64), "bin", u8p)):
        want = A.tail_reference(N, H, W)[key]
        left = A.blur_tile_row_mod(want, fill)
        assert HR.exact_failures(left, want) >= want.shape[0] * (H - A.BLUR_TILE) * min(W, A.BLUR_TILE) // 2, (N, H, W, key)
    for (N, H, W), planted in (((1, 13, 13), "clamp"), ((3, 13, 64), "clamp"), ((1, 20, 77), "cols_first"), ((1, 129, 130), "cols_first"), ((1, 63, 65), "clamp")):
        ref = A.tail_reference(N, H, W)
        taps = HR.gaussian_taps(A.TAPS_F32)
        got = np.stack([A.blur_planted(m.astype(np.float32), taps, planted) for m in ref["stack"]])
        assert HR.exact_failures(got, ref["blur"]) > 0, (N, H, W, planted)
    for (N, H, W) in ((3, 13, 13), (1, 64, 13), (3, 129, 130)):                                        # the clamped border through the binarisation
        ref = A.tail_reference(N, H, W)
        taps = HR.gaussian_taps(A.TAPS_U8)
        got = np.stack([np.where(np.rint(A.blur_planted(u.astype(np.float32), taps, "clamp")).clip(0, 255) > 4, 255, 0).astype(np.uint8) for u in ref["bin_in"]])
        assert HR.exact_failures(got, ref["bin"]) > 0, (N, H, W)
    for (N, H, W) in ((3, 13, 64), (3, 63, 65), (3, 20, 77), (3, 129, 130)):
        ref = A.tail_reference(N, H, W)
        assert HR.exact_failures(A.nms_across_the_seam(ref["nms_in"]), ref["nms"]) > 0, (N, H, W)


def test_planted_errors_are_rejected_image_prep():
    # v * (1 / 255f) against v / 255f over the 256 bytes: kept as a planted error only because it moves a byte
    v = torch.arange(256, dtype=F32)
    a, b = v / 255.0, v * torch.tensor(1.0 / 255.0, dtype=F32)
    moved = {dt: int((a.to(dt) != b.to(dt)).sum()) for dt in A.DTYPES}
    print("ANNOT-HOST v * (1 / 255f) moves %s of the 256 bytes" % ", ".join("%d (%s)" % (n, A.DT_NAME[dt]) for dt, n in moved.items()))
    assert moved[F32] > 0
    rows = [(A.pick(A.PREP, kind="h", dt=F32), "no_h_clamp"), (A.pick(A.PREP, Hin=17, dt=F16), "no_h_clamp"), (A.pick(A.PREP, Hin=17, dt=F32), "vertical_first"),
            (A.pick(A.PREP, Hin=9, dt=BF16), "vertical_first"), (A.pick(A.PREP, Hin=255, dt=F32), "vertical_first"), (A.pick(A.PREP, kind="v", dt=F16), "no_round"),
            (A.pick(A.PREP, Win=2048, dt=F32), "no_round"), (A.pick(A.PREP, kind="neither", dt=F32), "mul_inv255"), (A.pick(A.PREP, Hin=255, dt=F32), "mul_inv255"),
            (next(c for c in A.PREP if c.F == 3 and c.rep == 2), "replica_index"), (next(c for c in A.PREP if c.F == 3 and c.rep == 3), "replica_index"),
            (A.pick(A.PREP, kind="h", dt=F16), "kk_stride"), (A.pick(A.PREP, Hin=2048, dt=BF16), "kk_stride"), (A.pick(A.PREP, Hin=17, dt=BF16), "kk_stride"),
            (next(c for c in A.PREP if c.cfg == 2 and c.kind == "both"), "cfg_missing"), (next(c for c in A.PREP if c.cfg == 2 and c.kind == "one"), "cfg_missing")]
    assert {p for _, p in rows} == {"no_h_clamp", "vertical_first", "no_round", "mul_inv255", "replica_index", "kk_stride", "cfg_missing"}
    for c, planted in rows:
        want = A.prep_expected(c)
        n = A.prep_differs(A.prep_emulate(c, planted), want)
        assert n > 0, (c.id, planted)
        if planted == "cfg_missing":
            assert n == want[0].numel()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    rows = A.refusals(0x10000, 0x10002)
    named = {r[0] for r in rows}
    assert len(named) == len(rows) >= 24
    assert {"hed stem W % 4", "pidi stem W % 4", "pool_proj odd H", "pool_proj C = 96", "hed fuse H % 16", "blur_f32 H <= radius", "blur_u8_bin H <= radius",
            "hed fuse misaligned out", "pidi fuse misaligned out", "prep tables for an axis that is not resampled", "prep no tables for a resampled width",
            "prep cfg = 3", "prep null tmp"} <= named
    for name, sym, args, msg in rows:
        rc = getattr(lib, sym)(*args, ctypes.c_void_p(0))
        err = (lib.ctrl_last_error() or b"").decode()
        assert rc != 0 and msg in err, (name, rc, err)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle is Pillow, at every size of the table; the pass order on a tall sliver
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_is_pillow_at_every_table_size():
    PIL = pytest.importorskip("PIL.Image")
    sizes = sorted({(c.Hin, c.Win, c.H, c.W) for c in A.PREP})
    assert len(sizes) == 12
    for Hin, Win, H, W in sizes:
        for img in A.prep_frames(Hin, Win, 3):
            ref = np.asarray(PIL.fromarray(img, "RGB").resize((W, H), resample=PIL.Resampling.LANCZOS))
            got = O.pil_resize_lanczos(img, W, H)
            assert got.shape == ref.shape and np.array_equal(got, ref), "%dx%d -> %dx%d: %d bytes differ" % (Hin, Win, H, W, int((got != ref).sum()))


def test_pillow_pass_order_on_a_tall_sliver():
    """1000 x 3 -> 8 x 8: the installed Pillow equals the oracle's two passes in one of the two orders (which one is
    Pillow's private choice; prepare_images stays horizontal first)"""
    PIL = pytest.importorskip("PIL.Image")
    import PIL as pil_pkg
    img = A.rand_img(1000, 3, 4)
    ref = np.asarray(PIL.fromarray(img, "RGB").resize((8, 8), resample=PIL.Resampling.LANCZOS))
    hv = O._resample_axis(O._resample_axis(img, 8, 1), 8, 0)
    vh = O._resample_axis(O._resample_axis(img, 8, 0), 8, 1)
    print("ANNOT-HOST Pillow %s at 1000x3 -> 8x8: %s (the two orders differ in %d of %d bytes)" % (
        pil_pkg.__version__, "vertical first" if np.array_equal(ref, vh) else "horizontal first", int((hv != vh).sum()), hv.size))
    assert np.array_equal(ref, hv) or np.array_equal(ref, vh)
