"""Self-test of the helper-kernel checks (tests/helper_forms.py), no GPU: the tables hold the edges they declare (asserted from constants
restated from csrc/elementwise.hip, csrc/unet.hip and csrc/vae.hip), the fp32 emulations of the kernels stay within the bounds (at most
0.5 of them where a constant was calibrated, and above 0.5 one power of two lower), every planted error is rejected on a named case, the
phase and GEGLU restatements agree with independent formulations, and the entry points refuse what they must before any launch."""
import ctypes

import torch
import torch.nn.functional as Fn

import helpers  # noqa: F401
import helper_forms as H

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# the tables hold the declared edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_tables_hold_the_declared_edges():
    assert (H.TILE_C, H.TILE_P, H.THREADS, H.GRID_CAP, H.LS_MT, H.LS_COLS, H.LS_KTRIP, H.CO_LANES, H.CO_PIX) == (32, 64, 256, 8192, 8, 4, 512, 4, 64)
    assert H.TRIP == 8192 * 256
    # transposes (nchw_to_nhwc_kernel, nhwc_to_nchw_kernel): one tile short by one, full, over by one, and more than two tiles, on both axes
    base = [c for c in H.TRANSPOSE if c.map is None and not c.special]
    assert {(c.N, c.C, c.HW) for c in base} == {(n, c, p) for n in (1, 3) for c in (1, 31, 32, 33, 70) for p in (1, 63, 64, 65, 130)}
    assert {c.C - H.TILE_C for c in base} >= {-1, 0, 1} and {c.HW - H.TILE_P for c in base} >= {-1, 0, 1}
    assert max(c.C for c in base) > 2 * H.TILE_C and max(c.HW for c in base) > 2 * H.TILE_P
    assert {(c.dt, c.scale) for c in base} == {(d, s) for d in H.DTYPES for s in H.TR_SCALES}
    maps = [c for c in H.TRANSPOSE if c.map]
    assert any(sorted(c.map) == list(range(c.N)) and list(c.map) != list(range(c.N)) for c in maps)          # a permutation
    assert any(c.ndst > c.N and len(set(c.map)) == c.N and max(c.map) == c.ndst - 1 for c in maps)           # a scatter with unmapped images
    assert {c.dt for c in maps} == set(H.DTYPES)
    # avgpool (avgpool_kernel)
    assert {c.shape for c in H.AVGPOOL} == set(H.AP_SHAPES) and {c.NC for c in H.AVGPOOL} == {1, 5} and {c.dt for c in H.AVGPOOL} == set(H.DTYPES)
    assert {(s[0] // s[2], s[1] // s[3]) for s in H.AP_SHAPES} == {(1, 1), (3, 2), (8, 8), (2, 2)}
    n2 = H.AP_SECOND.NC * H.AP_SECOND.shape[2] * H.AP_SECOND.shape[3]
    assert H.TRIP < n2 < 2 * H.TRIP and H.AP_REFUSED[0] % H.AP_REFUSED[2] != 0
    # sincos (sincos_kernel): one workgroup of 256 holds N * dim / 2 up to 256; 3 * 160 needs two
    assert {(c.N, c.t_count, c.dim) for c in H.SINCOS} == {(1, 1, d) for d in (2, 6, 320)} | {(3, t, d) for t in (1, 3) for d in (2, 6, 320)}
    assert any(c.N * c.dim // 2 > H.THREADS for c in H.SINCOS) and set(H.SC_TS) == {0.0, 1.0, 250.5, 999.0}
    # linear_small (linear_small_kernel<8>, linear_small_group_kernel)
    assert {(c.M, c.N, c.K) for c in H.LINEAR} == {(m, n, k) for m in H.LS_MS for n in H.LS_NS for k in H.LS_KS}
    assert {m - H.LS_MT for m in H.LS_MS} >= {-1, 0, 1} and max(H.LS_MS) > 2 * H.LS_MT
    assert {n - H.LS_COLS for n in H.LS_NS} >= {-1, 0, 1} and {n % H.LS_COLS for n in H.LS_NS} >= {0, 1, 3}
    assert {k - H.LS_KTRIP for k in H.LS_KS} >= {-8, 0, 8} and max(H.LS_KS) > 2 * H.LS_KTRIP and min(H.LS_KS) == 8
    assert {(c.bias, c.in_silu, c.out_silu) for c in H.LINEAR} == {(a, b, d) for a in (False, True) for b in (False, True) for d in (False, True)}
    for k in H.LS_KS:
        assert {(c.in_silu, c.out_silu) for c in H.LINEAR if c.K == k} == {(b, d) for b in (False, True) for d in (False, True)}
    # blend (blend_kernel)
    assert {(c.xs, c.xt, c.y) for c in H.BLEND} == {(a, b, y) for a in (F16, F32) for b in (F16, F32) for y in (F16, F32)}
    assert {c.chunks - H.THREADS for c in H.BLEND} >= {-1, 1} and {c.mix for c in H.BLEND} == {0.0, 0.3, -20.0, 20.0}
    assert H.TRIP < H.BL_SECOND_CHUNKS < 2 * H.TRIP
    # add_rowvec (add_rowvec_kernel)
    assert {(c.C, c.rows_per_img, c.vmod) for c in H.ADDV} == {(c, r, v) for c in (8, 328) for r in (1, 5) for v in (1, 2, 3)}
    for c in H.ADDV:
        imgs = -(-c.M // c.rows_per_img)
        assert c.vmod == 1 or imgs % c.vmod != 0, c.id
        assert int(H.addv_index(c.M, c.rows_per_img, c.vmod).max()) == c.vmod - 1 and imgs > c.vmod          # the wrap runs
    assert any(c.x != c.y for c in H.ADDV) and any(c.inplace for c in H.ADDV) and {c.x for c in H.ADDV} == {F16, F32} == {c.y for c in H.ADDV}
    assert H.TRIP < H.AV_SECOND.M * (H.AV_SECOND.C // 8) < 2 * H.TRIP
    # merge (merge_kernel) and router (router_softmax_kernel)
    assert {(c.K, c.n, c.dt) for c in H.MERGE if not c.special} == {(k, n, d) for k in (1, 3, 8) for n in (1, 255, 257) for d in H.DTYPES}
    for c in H.MERGE:
        w = H.merge_widx(c)
        assert len(set(w)) == c.K and w != list(range(c.K)) and max(w) < c.E and c.E > c.K
    assert H.TRIP < H.MG_SECOND_N < 2 * H.TRIP
    assert {(c.E, c.R) for c in H.ROUTER} == {(e, r) for e in (1, 3, 16) for r in (1, 64, 65)} and {c.mask for c in H.ROUTER} == set(H.RT_MASKS)
    assert any(c.equal for c in H.ROUTER) and all(H.router_problem(c)[0] is None for c in H.ROUTER if c.equal)
    assert float(H.router_problem(next(c for c in H.ROUTER if c.E == 16 and c.mask == "none" and not c.equal))[0][0].abs().min()) == 50.0
    # packers
    assert {(c.Cout, c.Cin, c.taps) for c in H.PK_CONV} == {(a, b, t) for a in (1, 5) for b in (1, 3, 8) for t in (1, 3, 9)}
    assert {(c.Cout, c.Cin) for c in H.PK_DIRECT} == {(a, b) for a in (1, 5) for b in (1, 3, 8)}
    assert {(c.N, c.K) for c in H.PK_LINEAR} == {(n, k) for n in (5, 32, 64, 96) for k in (1, 8, 40)}
    assert {c.N for c in H.PK_LINEAR if c.geglu} == {32, 64, 96} and {(c.N, c.geglu) for c in H.PK_VEC} == {(1, False), (257, False), (64, True), (96, True)}
    for tab in (H.PK_CONV, H.PK_DIRECT, H.PK_LINEAR, H.PK_VEC):
        assert {c.dt for c in tab} == set(H.DTYPES)
    assert H.TRIP < H.PK_LINEAR_SECOND.N * H.PK_LINEAR_SECOND.K < 2 * H.TRIP
    for kind in H.OVF_KINDS:          # the `second` position lies beyond the first grid-stride trip of every packer
        r, c, t = H.OVF_SECOND[kind]
        assert H.TRIP < H.ovf_work_items(kind, H.OVF_SECOND[kind]) < 2 * H.TRIP
        first_out = {"conv": (r - 1) * t * c, "dup": (r - 1) * t * 2 * c, "phase": 16 * r * c - 1, "linear": (r - 1) * c}[kind]
        assert first_out >= H.TRIP, kind
    # unet_conv_out (unet_conv_out_kernel): chunks per lane 8 * 4 = 32 channels a round
    assert {(c.C, c.Cout, c.H, c.W) for c in H.CONV_OUT} >= {(a, b, h, w) for a in H.CO_CS for b in H.CO_COUTS for (h, w) in H.CO_MAPS}
    chunks = {C: [len(range(q * 8, C, 32)) for q in range(H.CO_LANES)] for C in H.CO_CS}
    assert chunks[16] == [1, 1, 0, 0] and chunks[24] == [1, 1, 1, 0] and chunks[32] == [1, 1, 1, 1] and chunks[40] == [2, 1, 1, 1] and chunks[320] == [10] * 4
    assert any(c.N * c.H * c.W == 105 for c in H.CONV_OUT) and any((c.N * c.H * c.W) % H.CO_PIX == 0 for c in H.CONV_OUT)
    assert {c.layout for c in H.CONV_OUT} == {H.NCHW, H.NCFHW, H.ROWS} and {c.F for c in H.CONV_OUT if c.layout == H.NCFHW} == {1, 3}
    assert all(c.N == 6 for c in H.CONV_OUT if c.layout == H.NCFHW) and {c.dt for c in H.CONV_OUT} == set(H.DTYPES)
    assert any(c.layout == H.ROWS and (c.C, c.Cout) == (16, 4) for c in H.CONV_OUT)
    for C in H.CO_CS:
        assert {(c.layout, c.dt) for c in H.CONV_OUT if c.C == C} >= {(l, d) for l in (H.NCHW, H.ROWS) for d in H.DTYPES} or C != 24
    # i2v_frames, vae_conv_in, vae_row_softmax
    assert {(c.B, c.F, c.HW, c.dt) for c in H.I2V} == {(b, f, p, d) for b in (1, 2) for f in (1, 3) for p in (1, 255, 257) for d in H.DTYPES}
    assert {(c.H, c.W, c.Cout, c.dt) for c in H.CONV_IN} == {(h, w, o, d) for (h, w) in ((1, 1), (1, 5), (7, 3), (17, 19)) for o in (16, 48, 128)
                                                           for d in H.DTYPES}
    assert any((c.H * c.W * c.Cout // H.CI_GROUP) % H.THREADS != 0 and c.H * c.W * c.Cout // H.CI_GROUP > H.THREADS for c in H.CONV_IN)
    assert {c.L for c in H.SOFTMAX} == {1, 63, 255, 256, 257, 1000} and {c.rows for c in H.SOFTMAX} == {1, 3} and {c.kind for c in H.SOFTMAX} == set(H.SM_KINDS)
    for L in H.SM_LS:
        assert {c.Lpad for c in H.SOFTMAX if c.L == L} == {L, -(-L // 64) * 64, L + 300}
        assert {c.kind for c in H.SOFTMAX if c.L == L and c.Lpad == L + 300} == set(H.SM_KINDS)
    assert all(c.Lpad - c.L > H.SM_THREADS for c in H.SOFTMAX if c.Lpad == c.L + 300)          # the fill loop's second trip
    assert {L - H.SM_THREADS for L in H.SM_LS} >= {-1, 0, 1}
    for tab in (H.TRANSPOSE, H.AVGPOOL, H.SINCOS, H.LINEAR, H.BLEND, H.ADDV, H.MERGE, H.ROUTER, H.PK_CONV, H.PK_DIRECT, H.PK_LINEAR, H.PK_VEC,
                H.CONV_OUT, H.I2V, H.CONV_IN, H.SOFTMAX):
        assert len({c.id for c in tab}) == len(tab)


# ---------------------------------------------------------------------------------------------------------------------------
# the emulations stay within their bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _with(name, value, fn):
    old = getattr(H, name)
    setattr(H, name, value)
    H.softmax_problem.cache_clear()
    try:
        return fn()
    finally:
        setattr(H, name, old)
        H.softmax_problem.cache_clear()


def _sincos_share(exact_only):
    w = 0.0
    for c in H.SINCOS:
        for which in range(4):
            _, ref, bound, ex = H.sincos_problem(c, which)
            r = (H.sincos_emulate(c, which).double() - ref).abs() / bound
            w = max(w, float((r[ex] if exact_only else r).max()))
    return w


def _blend_share():
    w = 0.0
    for c in H.BLEND:
        _, _, ref, bound = H.blend_problem(c)
        q = H.out_quantum(ref, c.y)
        w = max(w, float((((H.blend_emulate(c).double() - ref).abs() - 0.5 * q) / (bound - q)).max()))
    return w


def _router_share():
    return max(H.check(H.router_emulate(c), *H.router_problem(c)[2:4]) for c in H.ROUTER)


def _softmax_share():
    """the fp32 value before the store against the SM_K term alone"""
    w = 0.0
    for c in H.SOFTMAX:
        S, ref, bound, _ = H.softmax_problem(c.id)
        w = max(w, float(((H.softmax_emulate(c.id, keep32=True).double() - ref).abs() / H.softmax_term(S)).max()))
    return w


def test_emulations_stay_within_their_bounds():
    for name, fn, note in (("SC_C", lambda: _sincos_share(True), "cosf / sinf, the k = 0 columns"), ("SC_K", lambda: _sincos_share(False), "sincos, A = B"),
                           ("BL_K", _blend_share, "blend, beyond the output quantum"), ("RT_K", _router_share, "router"),
                           ("SM_K", _softmax_share, "vae_row_softmax, before the fp16 store")):
        k = getattr(H, name)
        share, lower = fn(), _with(name, k / 2, fn)
        print("HELPER-HOST %-4s = 2^%-3d share %.3f   one power of two lower: %.3f   (%s)" % (name, round(torch.log2(torch.tensor(k)).item()), share, lower, note))
        assert share <= 0.5 < lower, (name, share, lower)
    worst = {}

    def take(fam, v):
        worst[fam] = max(worst.get(fam, 0.0), v)

    for c in H.AVGPOOL:
        _, ref, bound = H.avgpool_problem(c)
        take("avgpool", H.check(H.avgpool_emulate(c), ref, bound))
    for c in H.LINEAR:
        if c.M in (1, 17) or c.K == 1288:
            take("linear_small", H.check(H.linear_emulate(c), *H.linear_reference(c)))
    for c in H.MERGE:
        if not c.special:
            take("merge", H.check(H.merge_emulate(c), *H.merge_problem(c)[3:5]))
    for c in H.CONV_OUT:
        if c.C <= 40 or (c.H, c.W) == (5, 7):
            take("unet_conv_out", H.check(H.conv_out_emulate(c.id), *H.conv_out_problem(c.id)[3:5]))
    for c in H.CONV_IN:
        take("vae_conv_in", H.check(H.conv_in_emulate(c.id), *H.conv_in_problem(c.id)[3:5]))
    for c in H.SOFTMAX:
        S, ref, bound, exact = H.softmax_problem(c.id)
        out = H.softmax_emulate(c.id)
        take("vae_row_softmax", H.check(out, ref, bound))
        if exact is not None:          # the constant row is fp16(1 / L) and the spike 1 beside exact zeros, bit for bit
            assert H.bits_equal(out, exact), c.id
    for fam, v in sorted(worst.items()):
        print("HELPER-HOST %-16s worst emulation / bound %.3f" % (fam, v))
        assert v <= 1.0, (fam, v)
    # the silu figure (tower_forms' e_quick at k = 1) holds for the fp32 restatement of silu_f on a grid
    x = torch.linspace(-30, 30, 600001, dtype=torch.float64).float()
    e = (H._silu32(x).double() - H.NF.silu64(x.double())).abs() / H._equick(x.double().abs(), x.double())
    print("HELPER-HOST silu fp32 emulation / e_quick: %.3f" % float(e.max()))
    assert float(e.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# every planted error is rejected on a named case
# ---------------------------------------------------------------------------------------------------------------------------
def test_planted_errors_are_rejected():
    # a last tile row / column left at poison; the image map ignored; one fp16 ulp on an exact case
    base = [c for c in H.TRANSPOSE if c.map is None and not c.special]
    for c, planted in ((H.pick(base, C=33, HW=65, dt=F16), "last_c_row"), (H.pick(base, C=70, HW=130, N=3), "last_p_col"),
                       (H.pick(H.TRANSPOSE, map=(2, 0, 1), C=33), "map_ignored"), (H.pick(H.TRANSPOSE, map=(4, 0, 2), C=70), "map_ignored")):
        good, bad = H.to_nchw_problem(c)[1], H.to_nchw_problem(c, planted)[1]
        assert H.bits_equal(good, H.to_nchw_problem(c)[1]) and not H.bits_equal(good, bad), (c.id, planted)
    want = H.to_nchw_problem(H.pick(base, C=33, HW=65, dt=F16))[1]
    assert not H.bits_equal(want, H.plus_one_ulp16(want, 7))
    want = H.to_nhwc_problem(H.pick(base, C=1, HW=1, N=3))[1]
    assert not H.bits_equal(want, H.plus_one_ulp16(want, 2))
    # a last chunk left at poison (blend: eight elements per thread)
    c = H.pick(H.BLEND, chunks=257, mix=0.3, y=F16)
    _, _, ref, bound = H.blend_problem(c)
    out = H.blend_emulate(c)
    assert H.check(out, ref, bound) <= 1.0
    out[-8:] = H.POISON[F16]
    assert H.check(out, ref, bound) > 1.0
    # vmod wrap off by one
    c = next(c for c in H.ADDV if c.vmod == 2 and c.rows_per_img == 5)
    assert not H.bits_equal(H.addv_problem(c)[2], H.addv_problem(c, "vmod_off_by_one")[2])
    # packers: tap order transposed at Cin = 3, the dup half shifted, the phase sets swapped, the GEGLU gate rows
    c = H.pick(H.PK_CONV, Cout=5, Cin=3, taps=9)
    w = H.pack_source(c, H.conv_w_shape(c))
    assert not H.bits_equal(H.pack_conv_expect(w), H.pack_conv_expect(w, "taps_transposed"))
    assert not H.bits_equal(H.pack_conv_dup_expect(w), H.pack_conv_dup_expect(w, "dup_shifted"))
    assert not H.bits_equal(H.pack_phase_expect(w), H.pack_phase_expect(w, "sets_swapped"))
    assert not H.bits_equal(H.pack_phase_expect(w), H.plus_one_ulp16(H.pack_phase_expect(w), 11))
    c = H.pick(H.PK_LINEAR, N=64, K=8, geglu=True)
    w = H.pack_source(c, (c.N, c.K))
    assert not H.bits_equal(H.pack_linear_expect(w, True), H.pack_linear_expect(w, True, "gate_from_32b"))
    # the range flag missed when only the last element is out of range
    for kind in H.OVF_KINDS:
        w = H.ovf_source(kind, H.OVF_SMALL[kind], F32, 7.0e4, "last")
        assert H.ovf_expected(kind, w) == 1 and H.ovf_expected(kind, w, "last_missed") == 0, kind
    # linear_small: a dropped last k trip, a dropped last column of a partly filled workgroup
    for c, planted in ((H.pick(H.LINEAR, M=9, N=5, K=520), "drop_last_trip"), (H.pick(H.LINEAR, M=1, N=333, K=1288), "drop_last_trip"),
                       (H.pick(H.LINEAR, M=9, N=5, K=520), "drop_last_col_of_wg")):
        assert H.check(H.linear_emulate(c, planted), *H.linear_reference(c)) > 1.0, (c.id, planted)
    # conv_out: the last live lane's chunk dropped at C = 24; NCFHW written as NCHW
    cid = next(c.id for c in H.CONV_OUT if c.C == 24 and c.H * c.W > 1)
    assert H.check(H.conv_out_emulate(cid, "drop_last_lane"), *H.conv_out_problem(cid)[3:5]) > 1.0
    cid = next(c.id for c in H.CONV_OUT if c.layout == H.NCFHW and c.F == 3 and c.Cout > 1)
    ref, bound = H.conv_out_problem(cid)[3:5]
    assert H.check(H.conv_out_emulate(cid, "ncfhw_as_nchw").reshape(ref.shape), ref, bound) > 1.0
    # vae_conv_in: the last thread's channel group unwritten
    cid = "ci-17x19-Co48-f32"
    assert H.check(H.conv_in_emulate(cid, "last_group_unwritten"), *H.conv_in_problem(cid)[3:5]) > 1.0
    # softmax: the maximum over the first 256 entries only
    for L in (257, 1000):
        cid = H.pick(H.SOFTMAX, L=L, kind="step").id
        assert H.check(H.softmax_emulate(cid, "max_first_256"), *H.softmax_problem(cid)[1:3]) > 1.0, cid
        assert H.check(H.softmax_emulate(cid), *H.softmax_problem(cid)[1:3]) <= 1.0, cid
    # router: the mask reaches the maximum but not the sum
    c = H.pick(H.ROUTER, E=3, R=65, mask="one", equal=False)
    _, _, ref, bound, dead = H.router_problem(c)
    out = H.router_emulate(c, "mask_not_in_sum")
    assert H.check(out, ref, bound) > 1.0 and bool((out[:, dead] != 0).any())
    assert H.check(H.router_emulate(c), ref, bound) <= 0.5 and bool((H.router_emulate(c)[:, dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the phase and GEGLU restatements against independent formulations
# ---------------------------------------------------------------------------------------------------------------------------
def test_phase_pack_is_the_conv_over_the_upsampled_map():
    """fp64: the four 2x2 phase convs built from the restated phase sums equal conv2d(nearest_x2(x), w, padding = 1)"""
    g = torch.Generator().manual_seed(5)
    Cout, Cin, Hs, Ws = 5, 3, 4, 6
    x = torch.randn(2, Cin, Hs, Ws, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    want = Fn.conv2d(Fn.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    ph = H.phase_sums(w, torch.float64)                                   # [2a + b][Cout][2ty + tx][Cin]
    xp = Fn.pad(x, (1, 1, 1, 1))
    got = torch.zeros_like(want)
    for a in (0, 1):
        for b in (0, 1):
            k = ph[2 * a + b].reshape(Cout, 2, 2, Cin).permute(0, 3, 1, 2)          # [Cout][Cin][ty][tx]
            # output pixel (2i + a, 2j + b) reads the source rows i + a - 1 + ty: in the padded map rows i + a + ty
            got[:, :, a::2, b::2] = Fn.conv2d(xp[:, :, a:a + Hs + 1, b:b + Ws + 1], k)
    assert float((got - want).abs().max()) < 1e-12
    bad = H.phase_sums(w, torch.float64, "sets_swapped")
    assert float((bad - ph).abs().max()) > 1e-3


def test_geglu_row_order_is_a_bijection_that_pairs_hidden_and_gate():
    for N in (32, 64, 96, 4096):
        rows = [H.geglu_row(p, N) for p in range(N)]
        assert sorted(rows) == list(range(N))
        for blk in range(N // 32):
            for j in range(16):
                assert rows[32 * blk + j] == 16 * blk + j and rows[32 * blk + 16 + j] == N // 2 + 16 * blk + j
        if N > 32:
            assert sorted(H.geglu_row(p, N, "gate_from_32b") % N for p in range(N)) != list(range(N))
    v = torch.arange(96.0)
    assert H.pack_vec_expect(v, True)[16:32].tolist() == list(range(48, 64)) and H.pack_vec_expect(v, False).tolist() == v.tolist()


def test_range_flag_restatement():
    """the guard is on the fp32 value: 65519 would round to 65504 in fp16 and is flagged all the same"""
    assert float(torch.tensor(65519.0).half()) == 65504.0
    for dt, rows in H.OVF_VALUES.items():
        for value, want in rows:
            assert float(torch.tensor(value).to(dt).float()) == value or value != value          # representable in the source type
            for kind in H.OVF_KINDS:
                for where in ("first", "last"):
                    assert H.ovf_expected(kind, H.ovf_source(kind, H.OVF_SMALL[kind], dt, value, where)) == want, (kind, dt, value, where)
    for dt in (F32, BF16):
        w = H.ovf_phase_sum_source(dt)
        assert H.ovf_expected("dup", w) == 0 and H.ovf_expected("conv", w) == 0 and H.ovf_expected("phase", w) == 1
        assert float(w.float().abs().max()) <= H.FP16_MAX


def test_the_smallest_plan_has_the_weight_the_range_test_edits():
    import ctrl_adapter_amd as P
    from vae_encoder_ref import TINY
    assert H.PLAN_WEIGHT in P.AutoencoderKLEncoder(**TINY).state_dict()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    rows = H.refusals(0x10000, 0x10002)
    assert len({r[0] for r in rows}) == len(rows) >= 30
    for name, sym, args, msg in rows:
        rc = getattr(lib, sym)(*args, ctypes.c_void_p(0))
        err = (lib.ctrl_last_error() or b"").decode()
        assert rc != 0 and msg in err, (name, rc, err)
