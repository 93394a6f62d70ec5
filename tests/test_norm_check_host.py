"""Host self-test of tests/norm_forms.py (no GPU): the tables are complete, the fp32 emulation of every kernel stays within half the
bound on every case, the bound rejects every planted error on every case it applies to, every `spike` case has tail rows that decide
its statistics, and the argument checks of the streaming ops refuse before any launch."""
import ctypes

import pytest
import torch

import norm_forms as nf


@pytest.fixture(scope="module")
def lib():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    return _lib.lib()


def _halves(c):
    P = nf.gn_problem(c)
    for col0, ref, bound in P.refs:
        yield P.x[:, :, col0:col0 + c.C].double(), P.gamma[col0:col0 + c.C], P.beta[col0:col0 + c.C], ref, bound, col0


def _beyond(out, ref, bound):
    return bool(((out - ref).abs() > bound).any())


# ------------------------------------------------------------------------------------------------------------------------------------
def test_table_is_complete(lib):
    from ctrl_adapter_amd import ops
    every = nf.GN + nf.FUSED + nf.LN + nf.LN_ADD
    names = [c.name for c in every]
    assert len(set(names)) == len(names)
    # every kernel template instance
    ran = {k for c in every for k in nf.kernel_of(c)}
    assert ran == set(nf.KERNELS), ran ^ set(nf.KERNELS)
    # every NCH with both sides of each boundary, in both dtypes, plain and with the added vector
    for tab in (nf.LN, nf.LN_ADD):
        assert {(nf.ln_nch(c.C), c.dt) for c in tab} == {(n, d) for n in (1, 2, 4) for d in ("f16", "f32")}
    assert {512, 520, 1024, 1032} <= {c.C for c in nf.LN} and [nf.ln_nch(C) for C in (512, 520, 1024, 1032)] == [1, 2, 2, 4]
    # the declared launch shapes are the launchers'; every chunk count the reduction has a path for appears
    for c in nf.GN:
        assert ops.gn_launch_shape(c.imgs, c.rows, c.C, 0) == tuple(c.stats), (c.name, c.stats)
        assert ops.gn_launch_shape(c.imgs, c.rows, c.C, 1) == tuple(c.apply), (c.name, c.apply)
        assert nf.mirror_launch_shape(c.imgs, c.rows, c.C, 0) == tuple(c.stats)
    for dt in ("f16", "f32"):
        got = {ops.gn_launch_shape(c.imgs, c.rows, c.C, 0)[1] for c in nf.GN if c.dt == dt}
        want = set(nf.GN_CHUNK_COUNTS) - ({96} if dt == "f32" else set())
        assert want <= got, (dt, want - got)
    big = [c for c in nf.GN if c.imgs * c.rows * c.C > 2 ** 21]
    assert len(big) == 1 and tuple(big[0].stats) == (11, 96)           # one large case: it leaves the 8 rpi floor
    # rows = 1 .. 7 (mod 8) at rpi = 1, both dtypes
    assert {(c.rows % 8, c.dt) for c in nf.GN if c.C == 1280 and c.rows < 16 and not c.layout} >= {(r, d) for r in range(1, 8) for d in ("f16", "f32")}
    # every layout argument non-default at least once, on three geometries and in both dtypes
    for lay in nf.LAYOUTS:
        assert {(c.C, c.halves, c.dt) for c in nf.GN if c.layout == lay} == {(C, h, d) for C, h in ((320, False), (1280, False), (1280, True))
                                                                             for d in ("f16", "f32")}, lay
    # every geometry has a spike case in both dtypes (and the other three kinds)
    for nm, C, G, hv in nf.GEOMETRIES:
        mine = [c for c in nf.GN if (c.C, c.G, c.halves) == (C, G, hv) and not c.layout]
        assert {c.dt for c in mine if c.kind == "spike"} == {"f16", "f32"}, nm
        assert {c.kind for c in mine} == {"spike", "plain", "offset", "flat"}, nm
    assert all(c.dt == "f32" for c in every if c.kind == "offset")
    # the fused form: rows around the 102 row lanes and 4 x 102, the largest map of each dtype
    for C in (320, 640, 1280, 2560):
        for dt in ("f16", "f32"):
            assert {1, 101, 102, 103, 407, 408, 409} <= {c.rows for c in nf.FUSED if c.C == C and c.dt == dt}
    assert {(c.rows, c.dt) for c in nf.FUSED} >= {(3276, "f16"), (1638, "f32")}
    for dt, code in (("f16", 1), ("f32", 0)):
        m = nf.fused_max_rows(dt)
        for C in (320, 640, 1280, 2560):
            assert lib.ctrl_op_gn_fused_applies(code, m, C, 32) == 1 and lib.ctrl_op_gn_fused_applies(code, m + 1, C, 32) == 0
        assert lib.ctrl_op_gn_fused_applies(code, 64, 160, 32) == 0          # 16 groups per 80-channel block: more than the 8 it holds
    # layernorm_add: the three (rows_per_img, vmod), M no multiple of their product
    assert {(c.rows_per_img, c.vmod) for c in nf.LN_ADD} == {(1, 1), (7, 3), (5, 2)}
    assert all(c.M % (c.rows_per_img * c.vmod) != 0 or c.vmod == 1 for c in nf.LN_ADD)


def test_launch_shape_query_refuses_bad_shapes(lib):
    a, b = ctypes.c_int(), ctypes.c_int()
    for args in ((0, 4, 320, 0), (1, 0, 320, 0), (1, 4, 4, 0), (1, 4, 324, 0), (1, 4, 2056, 0), (1, 4, 320, 2)):
        assert lib.ctrl_gn_launch_shape(*args, ctypes.byref(a), ctypes.byref(b)) != 0, args
    assert lib.ctrl_gn_launch_shape(1, 4, 320, 0, None, ctypes.byref(b)) != 0


# ------------------------------------------------------------------------------------------------------------------------------------
def test_emulation_stays_within_half_the_bound():
    worst, used = {}, {}
    for tab, fam in ((nf.GN, "gn_stats + gn_apply"), (nf.FUSED, "gn_fused")):
        for c in tab:
            for x, gamma, beta, ref, bound, _ in _halves(c):
                err = (nf.emulate_gn(c, x.float(), gamma, beta).double() - ref).abs()
                r = float((err / bound).max())
                key = fam + (" offset" if c.kind == "offset" else "")
                worst[key] = max(worst.get(key, 0.0), r)
                used[key] = max(used.get(key, 0.0), nf.stat_part(err, ref, bound))
                assert r <= 0.5, (c.name, r)
    for c in nf.LN + nf.LN_ADD:
        P = nf.ln_problem(c)
        err = (nf.emulate_ln(P.xsum if c.add else P.x, P.gamma, P.beta).double() - P.ref).abs()
        r = float((err / P.bound).max())
        worst["layernorm"] = max(worst.get("layernorm", 0.0), r)
        used["layernorm"] = max(used.get("layernorm", 0.0), nf.stat_part(err, P.ref, P.bound))
        assert r <= 0.5, (c.name, r)
    for k, v in sorted(worst.items()):
        print("NORM-EMU %-28s worst emulated err/bound %.3f, statistics term used %.3f (GN_K = %g, LN_K = %g)" % (k, v, used[k], nf.GN_K, nf.LN_K))
        assert used[k] <= 0.5, (k, used[k])                  # what decides the constants: at half of them (one power of two less) this fails


# ------------------------------------------------------------------------------------------------------------------------------------
def test_every_spike_row_decides_the_statistics():
    """planted error 1, one tail row dropped from the statistics: for EVERY spiked row of every `spike` case, the result normalised with
    sums that miss that row leaves the bound somewhere (looked for in the row's own group; a one-row image has no row to drop)"""
    checked = 0
    for c in nf.GN + nf.FUSED:
        if c.kind != "spike" or c.rows < 2:
            continue
        P = nf.gn_problem(c)
        cg = c.C // c.G
        assert P.spikes, c.name
        for x, gamma, beta, ref, bound, col0 in _halves(c):
            xg = x.reshape(c.imgs, c.rows, c.G, cg)
            rs, rss = xg.sum(3), (xg * xg).sum(3)                  # per (image, row, group)
            s, ss = rs.sum(1), rss.sum(1)
            for i, r, ch in P.spikes:
                if not col0 <= ch < col0 + c.C:
                    continue
                g = (ch - col0) // cg
                sl = slice(g * cg, (g + 1) * cg)
                out, _ = nf.gn_out(x[i:i + 1, :, sl], (s[i, g] - rs[i, r, g]).reshape(1, 1), (ss[i, g] - rss[i, r, g]).reshape(1, 1),
                                   (c.rows - 1) * cg, gamma[sl], beta[sl], 1, c.silu)
                assert _beyond(out, ref[i:i + 1, :, sl], bound[i:i + 1, :, sl]), "%s: dropping row %d of image %d is invisible" % (c.name, r, i)
                checked += 1
    assert checked > 1000


def _mutants(c):
    """(what, result) per planted error that applies to GroupNorm case `c`, one half at a time"""
    n = c.rows * (c.C // c.G)
    halves = list(_halves(c))
    for h, (x, gamma, beta, ref, bound, _) in enumerate(halves):
        s, ss = nf.gn_sums(x, c.G)
        if c.G > 1:
            sh = nf.gn_sums(torch.roll(x, -1, 2), c.G)                   # group g = channels g cg + 1 .. (g + 1) cg + 1
            yield "group boundary shifted by one channel", nf.gn_out(x, sh[0], sh[1], n, gamma, beta, c.G, c.silu)[0], ref, bound
        if c.silu:
            yield "SiLU omitted", nf.gn_out(x, s, ss, n, gamma, beta, c.G, False)[0], ref, bound
        if c.halves:
            og, ob = halves[1 - h][1], halves[1 - h][2]
            yield "gamma and beta of the other half", nf.gn_out(x, s, ss, n, og, ob, c.G, c.silu)[0], ref, bound
        if c.layout == "sharded":
            ra = nf.shard_rows(c.rows)
            out = torch.cat([nf.gn_out(p, s, ss, p.shape[1] * (c.C // c.G), gamma, beta, c.G, c.silu)[0] for p in (x[:, :ra], x[:, ra:])], 1)
            yield "stat_rows taken as rows_per_img", out, ref, bound


def test_bound_rejects_planted_groupnorm_errors():
    seen = {}
    for c in nf.GN + nf.FUSED:
        for what, out, ref, bound in _mutants(c):
            assert _beyond(out, ref, bound), "%s: %s passes the bound" % (c.name, what)
            seen[what] = seen.get(what, 0) + 1
    assert set(seen) == {"group boundary shifted by one channel", "SiLU omitted", "gamma and beta of the other half",
                         "stat_rows taken as rows_per_img"}, seen
    print("NORM-MUTANTS", seen)


def test_bound_rejects_planted_layernorm_errors():
    n_idx = n_pad = 0
    for c in nf.LN_ADD:
        if c.vmod == 1:
            continue
        P = nf.ln_problem(c)
        wrong = nf._round(P.x + P.addv[torch.arange(c.M) % c.vmod], c.dt)             # row % vmod instead of (row / rows_per_img) % vmod
        assert _beyond(nf.ln_reference(wrong, P.gamma, P.beta)[0], P.ref, P.bound), c.name
        n_idx += 1
    for c in nf.LN:
        if not c.wide:
            continue
        P = nf.ln_problem(c)
        out = nf.ln_reference(P.x, P.gamma, P.beta, count=c.C + 16)[0]                # statistics over the padded row (pads as zeros)
        assert _beyond(out, P.ref, P.bound), c.name
        n_pad += 1
    assert n_idx == 12 and n_pad == len(nf.LN_C) * 4 * 2


# ------------------------------------------------------------------------------------------------------------------------------------
def test_streaming_ops_refuse_zero_divisors_and_null_pointers(lib):
    """each of these used to reach the device (a division by zero there); now a CTRL_CHECK before any launch"""
    p = 0x1000                      # never dereferenced: every call below is refused on the host
    F16c = 1

    def refused(rc, text):
        assert rc != 0 and text in lib.ctrl_last_error().decode(), (rc, lib.ctrl_last_error())

    refused(lib.ctrl_op_add_rowvec(p, F16c, p, 8, p, F16c, 4, 8, 0, 1, None), "rows_per_img and vmod")
    refused(lib.ctrl_op_add_rowvec(p, F16c, p, 8, p, F16c, 4, 8, 1, 0, None), "rows_per_img and vmod")
    for args in ((None, F16c, p, 8, p), (p, F16c, None, 8, p), (p, F16c, p, 8, None)):
        refused(lib.ctrl_op_add_rowvec(*args, F16c, 4, 8, 1, 1, None), "add_rowvec: null pointer")
    for bfl in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        refused(lib.ctrl_op_add_rowvec_clip(p, F16c, p, 8, p, F16c, *bfl, 8, None), "B, F and L")
    for args in ((None, F16c, p, 8, p), (p, F16c, None, 8, p), (p, F16c, p, 8, None)):
        refused(lib.ctrl_op_add_rowvec_clip(*args, F16c, 1, 1, 1, 8, None), "add_rowvec_clip: null pointer")
    refused(lib.ctrl_op_linear_small(p, 8, p, None, p, 4, 1, 0, 8, 0, 0, None), "N must be at least 1")
    for args in ((None, 8, p, None, p), (p, 8, None, None, p), (p, 8, p, None, None)):
        refused(lib.ctrl_op_linear_small(*args, 4, 1, 4, 8, 0, 0, None), "linear_small: null pointer")
    for fn in (lib.ctrl_op_gn_stats_group, lib.ctrl_op_gn_apply_group, lib.ctrl_op_gn_fused_group, lib.ctrl_op_layernorm_group):
        assert fn(None, 1, None) != 0 and fn(p, 0, None) != 0 and fn(p, 5, None) != 0
    assert lib.ctrl_op_linear_small_group(None, 1, None) != 0 and lib.ctrl_op_linear_small_group(p, 0, None) != 0
