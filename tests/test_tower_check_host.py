"""Self-test of the CLIP tower checks (tests/tower_forms.py), no GPU: the fp32 emulations of the kernels stay within the bounds (at most
0.5 of them where a constant was calibrated), every planted error is rejected on a named table case, the tables hold the edges they
declare (recomputed from constants restated from csrc/text_gemm.hip and csrc/text.hip), and the entry points refuse what they must
before any launch."""
import ctypes

import pytest
import torch

import helpers  # noqa: F401
import tower_forms as T

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# the tables hold the declared edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_gemm_table_holds_the_declared_edges():
    geo = {nk: T.gemm_geometry(*nk) for nk in T.GEMM_NK}
    assert [geo[nk][0] for nk in T.GEMM_NK] == [1, 1, 1, 1, 1, 2, 3, 2, 3, 1]
    assert any(N % 32 == 16 for N, _ in T.GEMM_NK)                                          # the n < N guard of a half-filled tile
    assert {K % 128 for _, K in T.GEMM_NK} >= {0, 32, 64, 96}                               # waves of 1, 2 and 3 k-steps
    assert any(K < 128 for _, K in T.GEMM_NK)
    assert geo[(32, 160)][1] == [(2, [4, 1, 0, 0])]                                         # nwaves < 4 with a one-step wave
    assert geo[(32, 544)][1] == [(4, [4, 4, 4, 4]), (1, [1, 0, 0, 0])]                      # a last split of a single k-step
    assert geo[(48, 1056)][1][2] == (1, [1, 0, 0, 0]) and geo[(64, 992)][1][1] == (4, [4, 4, 4, 3])
    assert geo[(32, 320)][1] == [(3, [4, 4, 2, 0])]
    assert geo[(48, 96)][1] == [(1, [3, 0, 0, 0])] and geo[(16, 32)][1] == [(1, [1, 0, 0, 0])]
    for nk in T.GEMM_NK:
        for nwaves, nsteps in geo[nk][1]:
            assert nwaves == sum(1 for n in nsteps if n > 0)                                # a wave is summed iff it owns a k-step
        assert sum(32 * sum(ns) for _, ns in geo[nk][1]) == nk[1]                            # every k is owned exactly once
        assert {c.M for c in T.GEMM if (c.N, c.K) == nk} >= {33, 77}
    for nk in T.GEMM_ALL_M:
        assert {c.M for c in T.GEMM if (c.N, c.K) == nk} == set(T.GEMM_MS)
    assert {(c.act, c.dt) for c in T.GEMM} == {(a, d) for a in (0, 2, 3) for d in T.DTYPES}
    assert {(c.bias, c.res) for c in T.GEMM} == {(a, b) for a in (False, True) for b in (False, True)}
    assert len({c.id for c in T.GEMM}) == len(T.GEMM)
    # the finish kernel alone
    assert {c.splits for c in T.FINISH} == {1, 2, 3} and {c.act for c in T.FINISH} == {0, 2, 3} and {c.dt for c in T.FINISH} == set(T.DTYPES)
    big = [c for c in T.FINISH if c.M * (c.N // 4) > T.FIN_GRID_BLOCKS * T.FIN_THREADS]
    assert len(big) == 1 and big[0].splits == 1 and big[0].M * (big[0].N // 4) < 2 * T.FIN_GRID_BLOCKS * T.FIN_THREADS
    assert all(c.N % 4 == 0 for c in T.FINISH)


def test_attention_table_holds_the_declared_edges():
    assert {c.L for c in T.ATTN} == set(T.ATTN_LS)
    kpads = {L: T.attn_geometry(L)[0] for L in T.ATTN_LS}
    assert set(kpads.values()) == {32, 64, 96, 128} and kpads[97] == 128 and kpads[96] == 96
    ntiles = {len(T.attn_geometry(L)[1]) for L in T.ATTN_LS}
    assert ntiles == set(range(1, 9))                                                       # key tiles 5 to 7 (and 8) run
    # a tile whose P needs the zero fill beyond nkt: an odd number of 16-key tiles
    assert any(nkt * 16 < nkp for L in T.ATTN_LS for (_, nkt, nkp) in T.attn_geometry(L)[1])
    assert T.attn_geometry(128)[1][-1] == (128, 8, 128) and T.attn_geometry(113)[1][-1] == (113, 8, 128)
    assert sorted({c.N * c.heads for c in T.ATTN}) == [1, 7, 8, 9, 20, 40] and {c.heads for c in T.ATTN} >= {1, 3, 20}
    for L in (17, 77, 128):
        got = {(c.N, c.heads, c.dld, c.dldo) for c in T.ATTN if c.L == L}
        assert got >= {(n, h, a, b) for (n, h) in T.ATTN_PAIRS for (a, b) in T.ATTN_STRIDES}
        assert {c.kind for c in T.ATTN if c.L == L} == set(T.ATTN_KINDS)
    for L in T.ATTN_LS:
        assert any(c.L == L and c.N * c.heads == 1 for c in T.ATTN)
    # the future kind: for a single pair the large keys start inside a query tile that holds a query below them
    for L in T.ATTN_LS:
        t = T.future_start(L, 0, 1)
        assert t == L == 1 or (1 <= t < L and t % 16 == 1) or L == 17 and t == 2, (L, t)
    for L in (17, 77, 128):
        assert len({T.future_start(L, p, 40) for p in range(40)}) >= min(16, L - 1)


def test_row_tables_hold_the_declared_edges():
    assert {c.C for c in T.ROWS} == set(T.ROW_CS)
    assert [T.text_row_kernel(C)[1] for C in T.ROW_CS] == [4] * 9 + [8] * 3 and T.text_row_kernel(1025) is None and T.text_row_kernel(2112) is None
    assert T.text_row_kernel(1024, True)[0] == "text_final_ext<4>" and T.text_row_kernel(1088, True)[0] == "text_final_ext<8>"
    for op in ("text_embed", "text_final", "text_final_ext", "vision_embed", "vision_cls_ln"):
        assert {(c.C, c.kind) for c in T.ROWS if c.op == op} >= {(C, k) for C in T.ROW_CS for k in T.ROW_KINDS}, op
    fin = [c for c in T.ROWS if c.op == "text_final"]
    assert {c.xdt for c in fin} == set(T.DTYPES) == {c.ydt for c in fin} and any(c.y_null for c in fin)
    assert {c.L for c in T.ROWS if c.op == "vision_embed"} == {2, 5}
    assert {c.outs for c in T.ROWS if c.op == "vision_cls_ln"} == {"both", "pooled", "pooled32"}
    assert len({c.id for c in T.ROWS}) == len(T.ROWS)
    for L in T.POOL_LS:
        names = [r[0] for r in T.pool_table(L)]
        assert len(set(names)) == len(names)
        for name, eos, ids, want in T.pool_table(L):
            assert len(ids) == L and T.pooled_index_ref(ids, eos) == want, (L, name)
            assert 2 not in ids and (eos == 2 or T.POOL_EOS not in ids or "eos" in name)
    assert {r[0] for r in T.pool_table(128)} >= {"argmax at 64", "argmax tie (5, 70)", "argmax tie (6, 70), one lane", "eos twice, one lane",
                                                 "eos twice, two lanes", "eos absent", "eos and a larger id elsewhere"}
    assert [T.resize_taps(a, b) for a, b in ((8, 8), (5, 12), (7, 9), (128, 4), (134, 4), (66, 3))] == [3, 3, 3, 63, 65, 43]
    assert T.resize_taps(T.RESIZE_REFUSED[0], T.RESIZE_REFUSED[2]) > T.RESIZE_MAX_TAPS


# ---------------------------------------------------------------------------------------------------------------------------
# the emulations stay within their bounds
# ---------------------------------------------------------------------------------------------------------------------------
def test_activation_constants():
    z = torch.linspace(-40, 40, 800001, dtype=torch.float64)
    s = torch.sigmoid(z)
    slope = float((s + z * s * (1 - s)).abs().max())
    print("TOWER-HOST largest slope of x sigmoid(k x): %.4f (SLOPE 1.1)" % slope)
    assert 1.09 < slope <= T.SLOPE[2]
    g = torch.distributions.Normal(0.0, 1.0)
    x = torch.linspace(-12, 12, 400001, dtype=torch.float64)
    gs = float((0.5 * (1 + torch.special.erf(x / 2 ** 0.5)) + x * g.log_prob(x).exp()).abs().max())
    assert 1.12 < gs <= T.SLOPE[3]
    # x sigmoid(1.702 x) in fp32 against the derived e_quick
    x = torch.linspace(-30, 30, 600001, dtype=torch.float64).float()
    err = (T.act_emul(x, 2).double() - T.act64(x.double(), 2)).abs()
    worst = float((err / T.act_err(x.double().abs(), x.double(), 2)).max())
    print("TOWER-HOST quick_gelu fp32 emulation / derived e_quick: %.3f" % worst)
    assert worst <= 1.0


def test_emulations_stay_within_their_bounds():
    worst = {}
    for c in T.GEMM:
        ref, bound = T.gemm_reference(c.id)
        worst["gemm act%d" % c.act] = max(worst.get("gemm act%d" % c.act, 0.0), T.check(T.gemm_emulate(c.id), ref, bound))
    for c in T.FINISH:
        p = T.finish_problem(c.id)
        r = T.check(T.finish_emulate(c.id), p["ref"], p["bound"])
        key = "finish act%d %s" % (c.act, T.DT_NAME[c.dt])
        worst[key] = max(worst.get(key, 0.0), r)
    for c in T.ATTN:
        p = T.attn_problem(c.id)
        out = T.attn_emulate(p["q"], p["k"], p["v"])
        worst["attn " + c.kind] = max(worst.get("attn " + c.kind, 0.0), T.check(out, p["ref"], p["bound"]))
        # row 0 of every prompt is V[0]
        assert torch.equal(p["ref"][:, :, 0], p["v"][:, :, 0].double())
    for c in T.PROJ:
        _, _, ref, bound = T.proj_problem(c)
        worst["proj"] = max(worst.get("proj", 0.0), T.check(T.proj_emulate(c), ref, bound))
    for k, v in sorted(worst.items()):
        print("TOWER-HOST emulated worst err/bound  %-18s %.3f" % (k, v))
        assert v <= 1.0, k
    # the calibrated constant of erff: at most 0.5 of the bound where only the activation remains (fp32 store), and minimal
    share = worst["finish act3 f32"]
    print("TOWER-HOST ERF_K = 2^%d: share %.3f" % (torch.log2(torch.tensor(T.ERF_K)).item(), share))
    assert share <= 0.5
    half = 0.0
    for c in T.FINISH:
        if c.act == 3 and c.dt == F32 and not c.res:
            p = T.finish_problem(c.id)
            half = max(half, T.check(T.finish_emulate(c.id), p["ref"], T.act_err(p["v"].abs(), p["v"], 3, T.ERF_K / 2) + 2.0 ** -140))
    x = torch.linspace(-12, 12, 2000001, dtype=torch.float64).float()
    grid = T.check(T.act_emul(x, 3), T.act64(x.double(), 3), T.act_err(x.double().abs(), x.double(), 3) + 2.0 ** -140)
    print("TOWER-HOST ERF_K: share on a grid over [-12, 12] %.3f; ERF_K / 2 would give %.3f on the table" % (grid, half))
    assert grid <= 0.5 and half > 0.5, "ERF_K is not the smallest power of two"


def _row_emulation_shares(kind, k):
    tot, share = 0.0, 0.0
    for C in T.ROW_CS:
        for per in ((4, 8) if C <= 1024 else (8,)):
            x, g, b = T.row_data(kind, 6, C, "host")
            y = T.row_ln_emulate(x, g, b, per)
            ref, _ = T.ln_ref(x, g, b, F32, kind)
            stat = k * T.U * (1.0 + torch.log2(torch.tensor(float(C)))) * (g.double().abs() * (1.0 + ((ref - b.double()) / g.double()).abs()) + b.double().abs())
            q = T.quantum(ref, F32)
            err = (y.double() - ref).abs()
            tot = max(tot, float((err / (q + stat)).max()))
            share = max(share, float(((err - 0.5 * q) / stat).max()))
    return tot, share


def test_row_ln_emulation_stays_within_half_the_bound():
    for kind in ("plain", "offset"):
        k = T.ln_k(kind)
        tot, share = _row_emulation_shares(kind, k)
        _, lower = _row_emulation_shares(kind, k / 2)
        print("TOWER-HOST row_ln %-6s K = 2^%d: worst err/bound %.3f, share of the statistics term %.3f (K / 2: %.3f)" % (
            kind, torch.log2(torch.tensor(k)).item(), tot, share, lower))
        assert tot <= 0.5 and share <= 0.5
        assert lower > 0.5, "the constant of `%s` is not the smallest power of two" % kind
    # flat rows: beta, bit for bit, in both instantiations
    for C in T.ROW_CS:
        x, g, b = T.row_data("flat", 2, C, "host")
        for per in ((4, 8) if C <= 1024 else (8,)):
            assert torch.equal(T.row_ln_emulate(x, g, b, per), b.expand(2, C))


# ---------------------------------------------------------------------------------------------------------------------------
# every planted error is rejected (the named case), and the same emulation without it passes (tested above)
# ---------------------------------------------------------------------------------------------------------------------------
GEMM_REJECTED_ON = {
    "drop_last_kstep_of_partial_wave": "N32-K160-M33",
    "nwaves_minus_one": "N32-K160-M77",
    "nwaves_plus_one": "N32-K512-M33",
    "drop_last_split": "N32-K544-M77",
    "zero_upper_half_tile": "N48-K1056-M33",
    "tail_rows_reuse_last": "N48-K1056-M77",
}


@pytest.mark.parametrize("planted", T.GEMM_PLANTED)
def test_gemm_planted_error_is_rejected(planted):
    ids = [c.id for c in T.GEMM if c.id.startswith(GEMM_REJECTED_ON[planted] + "-")]
    assert len(ids) == 1
    ref, bound = T.gemm_reference(ids[0])
    r = T.check(T.gemm_emulate(ids[0], planted), ref, bound)
    n = sum(T.check(T.gemm_emulate(c.id, planted), *T.gemm_reference(c.id)) > 1.0 for c in T.GEMM)
    print("TOWER-HOST planted %-34s on %-40s err/bound %.3g; rejected on %d of %d cases" % (planted, ids[0], r, n, len(T.GEMM)))
    assert r > 1.0


def _attn_id(L, kind, pairs=None):
    return [c.id for c in T.ATTN if c.L == L and c.kind == kind and (pairs is None or c.N * c.heads == pairs)][0]


ATTN_REJECTED_ON = {"mask_key_lt_q": (17, "diagonal"), "mask_off_past_L": (17, "plain"), "p_not_zeroed": (17, "diagonal")}


@pytest.mark.parametrize("planted", T.ATTN_PLANTED)
def test_attention_planted_error_is_rejected(planted):
    cid = _attn_id(*ATTN_REJECTED_ON[planted])
    p = T.attn_problem(cid)
    r = T.check(T.attn_emulate(p["q"], p["k"], p["v"], planted), p["ref"], p["bound"])
    print("TOWER-HOST planted %-34s on %-40s err/bound %.3g" % (planted, cid, r))
    assert r > 1.0
    if planted == "mask_key_lt_q":          # the diagonal kind loses the dominant key: every row from 1 on is wrong, not one element
        out = T.attn_emulate(p["q"], p["k"], p["v"], planted).double()
        bad = ((out - p["ref"]).abs() > p["bound"]).any(-1)
        assert bool(bad[..., 1:].all())


def test_future_keys_leaking_are_far_outside_the_bound():
    """a mask that lets ONE key after the query through (key <= q + 1) on the `future` cases: the error is orders of magnitude beyond the
    bound for the queries right below the large keys"""
    for cid in (_attn_id(77, "future", 1), _attn_id(128, "future", 40)):
        p = T.attn_problem(cid)
        q, k, v = p["q"], p["k"], p["v"]
        L = q.shape[2]
        s = (q.float() @ k.float().transpose(-1, -2)) * T.ATTN_C
        vis = torch.arange(L)[None, :] <= torch.arange(L)[:, None] + 1
        w = torch.softmax(s.masked_fill(~vis, float("-inf")).double() * 0.6931471805599453, -1)
        r = T.check((w @ v.double()).half(), p["ref"], p["bound"])
        print("TOWER-HOST one future key visible on %-40s err/bound %.3g" % (cid, r))
        assert r > 1e3


def test_row_and_pool_and_vt_planted_errors_are_rejected():
    # the variance over 256 * PER columns: C = 1000 (PER 4) and C = 1280 (PER 8)
    for C, per in ((1000, 4), (1280, 8)):
        x, g, b = T.row_data("plain", 6, C, "host")
        ref, bound = T.ln_ref(x, g, b, F32, "plain")
        r = T.check(T.row_ln_emulate(x, g, b, per, "variance_over_width"), ref, bound)
        print("TOWER-HOST planted variance_over_width on C = %d: err/bound %.3g" % (C, r))
        assert r > 1.0
    hit = {p: [] for p in T.POOL_PLANTED}
    for L in T.POOL_LS:
        for name, eos, ids, want in T.pool_table(L):
            for p in T.POOL_PLANTED:
                if T.pooled_index_ref(ids, eos, p) != want:
                    hit[p].append((L, name))
    print("TOWER-HOST planted pooled-index errors rejected on: %s" % {k: v[:3] for k, v in hit.items()})
    assert (77, "argmax tie (5, 70)") in hit["last_match"] and (128, "eos twice, one lane") in hit["last_match"]
    assert (65, "eos absent") in hit["eos_falls_back_to_argmax"]
    # vision_vt copying rows >= L: image 0 of N = 2 takes image 1's rows, the last image what follows the buffer (NaN guard rows)
    c = [c for c in T.VT if (c.L, c.Lkpad, c.C, c.N, c.qkv) == (33, 64, 32, 2, False)][0]
    v = torch.randn(c.N * c.L, c.C).half()
    good = T.vt_expected(v, c.N, c.L, c.C, c.Lkpad)
    bad = T.vt_expected(v, c.N, c.L, c.C, c.Lkpad, "copies_rows_past_L", after=torch.full((c.Lkpad, c.C), float("nan")).half())
    assert not torch.equal(good[0], bad[0]) and bool((good[:, :, c.L:] == 0).all()) and bool(torch.isnan(bad[1, :, c.L:]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# refusals that need no GPU: a non-zero return before any launch (the pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib as L_
    lib = L_.lib()
    P = ctypes.c_void_p(0x10000)          # 16-byte aligned, never dereferenced
    nul = ctypes.c_void_p(0)

    def refused(rc, word):
        assert rc != 0
        msg = lib.ctrl_last_error().decode()
        assert word in msg, msg

    refused(lib.ctrl_op_text_attn(P, 3 * 64, P, 64, 1, 129, 1, 0.125, nul), "L <= 128")
    refused(lib.ctrl_op_text_attn(P, 3 * 64 + 4, P, 64, 1, 16, 1, 0.125, nul), "ld % 8")
    for C in (1025, 2112):
        refused(lib.ctrl_op_text_embed(P, P, P, 10, 1, 2, C, P, P, P, 1e-5, P, nul, nul), "bad shape")
        refused(lib.ctrl_op_text_final_ln(P, 0, 2, C, P, P, 1e-5, P, 0, nul, 2, 2, nul, nul), "bad shape")
        refused(lib.ctrl_op_text_final_ln_ext(P, 0, 2, C, P, P, 1e-5, P, 0, P, 2, 2, P, P, nul), "bad shape")
    refused(lib.ctrl_op_vision_embed(P, P, P, 1, 2, 2049, P, P, P, P, 1e-5, P, P, nul), "bad shape")
    refused(lib.ctrl_op_vision_cls_ln(P, 1, 2, 2049, P, P, 1e-5, P, 0, P, nul), "bad shape")
    ws = lib.ctrl_text_gemm_ws_bytes(33, 48, 1056)
    assert ws == 3 * 33 * 48 * 4 and lib.ctrl_text_gemm_ws_bytes(1, 16, 32) == 64
    refused(lib.ctrl_op_text_gemm(P, P, nul, 33, 40, 1056, 0, nul, P, 0, P, ws, nul), "N % 16")
    refused(lib.ctrl_op_text_gemm(P, P, nul, 33, 48, 1040, 0, nul, P, 0, P, ws, nul), "K % 32")
    refused(lib.ctrl_op_text_gemm(P, P, nul, 33, 48, 1056, 0, nul, P, 0, P, ws - 4, nul), "workspace too small")
    refused(lib.ctrl_op_text_gemm(P, P, nul, 33, 48, 1056, 1, nul, P, 0, P, ws, nul), "act")
    refused(lib.ctrl_op_text_gemm_finish(P, 1, 4, 6, nul, 0, nul, 0, P, 0, 6, nul), "N % 4")
    refused(lib.ctrl_op_text_gemm_finish(P, 1, 4, 8, nul, 0, nul, 0, P, 0, 7, nul), "bad output")
    refused(lib.ctrl_op_text_gemm_finish(P, 1, 4, 8, nul, 0, P, 7, P, 0, 8, nul), "bad output")
    refused(lib.ctrl_op_vision_vt(P, 32, P, 1, 33, 32, 32, nul), "bad shape")          # Lkpad < L
    refused(lib.ctrl_op_vision_vt(P, 16, P, 1, 8, 32, 32, nul), "bad shape")           # ld < C
    refused(lib.ctrl_op_text_proj(P, P, 0, 4, 4, P, 0, nul), "bad argument")
    refused(lib.ctrl_op_text_store(P, P, 5, 4, nul), "bad argument")
    refused(lib.ctrl_op_text_store(P, P, 0, -1, nul), "n must be")
    H, W, OH, OW = T.RESIZE_REFUSED
    refused(lib.ctrl_op_clip_resize_aa(P, 0, 1, H, W, OH, OW, None, P, 0, nul), "more than 63 taps")
    refused(lib.ctrl_op_vision_patchify(P, 0, 1, 15, 14, None, P, 640, nul), "multiple of patch_size")
    refused(lib.ctrl_op_vision_patchify(P, 0, 1, 14, 14, None, P, 576, nul), "Kpad")
