"""Every kernel of csrc/norm.hip -- gn_stats_kernel, gn_apply_kernel, gn_fused_kernel, layernorm_kernel<1 | 2 | 4>, each for fp16 and fp32
input -- at its chunk, lane, stride and grouping edges, against the fp64 reference and the element-wise bound of tests/norm_forms.py
(whose host self-test is tests/test_norm_check_host.py).

Per case: inputs live inside NaN-filled surroundings (helpers.Guarded.inp: guard rows, and pad columns where the case has wider rows), results
inside a fixed bit pattern that must come back bit for bit (Guarded.out); the statistics buffer is followed by guard floats and its ticket
words must read zero after every launch.  Every test prints the worst |err| / bound it saw (PARITY lines); the worst over each kernel
family, the `offset` kind apart, is what DESIGN.md records.
"""
import pytest
import torch

import norm_forms as nf
from helpers import _POISON, Guarded, _bits

pytestmark = pytest.mark.gpu
DT = {"f16": torch.float16, "f32": torch.float32}


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


STAT_PART = [0.0]          # worst share of the statistics term used since the last _run_table / reset (norm_forms.stat_part)


def _close(out, ref, bound, what, rounds=True):
    """every element finite and within the bound of the fp64 reference; returns the worst |err| / bound"""
    o = out.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite results (a poisoned pad reached a kept element)" % (what, int((~torch.isfinite(o)).sum()))
    ratio = (o - ref).abs() / bound
    worst = float(ratio.max())
    if rounds:                                                   # (a bound of one fp16 quantum + the statistics term)
        STAT_PART[0] = max(STAT_PART[0], nf.stat_part((o - ref).abs(), ref, bound))
    if worst > 1.0:
        idx = tuple(int(v) for v in (ratio > 1.0).nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond the bound (worst err/bound %.2f); first at %s: got %.6g want %.6g bound %.3g" % (
            what, int((ratio > 1.0).sum()), ratio.numel(), worst, idx, float(o[idx]), float(ref[idx]), float(bound[idx])))
    return worst


def _poison_left(t, what):
    """a region of an output buffer no kernel may write still holds the fill pattern"""
    want = torch.full((), _POISON[t.dtype], dtype=t.dtype)
    assert bool((_bits(t) == _bits(want)).all()), "%s: written" % what


class Stats:
    """a zeroed statistics buffer of exactly the size the op asks for, followed by guard floats"""

    def __init__(self, ops, gpu, imgs, rows, C, G):
        self.n = ops.gn_stats_floats(imgs, rows, C, G)
        self.imgs, self.G = imgs, G
        self.buf = torch.zeros(self.n + 64, dtype=torch.float32, device=gpu)
        self.buf[self.n:] = _POISON[torch.float32]
        self.view = self.buf[:self.n]

    def sums(self):
        return self.view[:self.imgs * self.G * 2].clone()

    def check(self, what):
        torch.cuda.synchronize()
        _poison_left(self.buf[self.n:], what + ": floats past the statistics buffer")
        tickets = self.view[self.imgs * self.G * 2:self.imgs * self.G * 2 + self.imgs].view(torch.int32)
        assert bool((tickets == 0).all()), "%s: ticket words %s after the launch" % (what, tickets.tolist())


def _x_input(c, data, gpu):
    """data [imgs * rows][Cw] (Cw = 2 C for the halves form) inside NaN surroundings -> (Guarded, ldx as the descriptor takes it)"""
    pad = 8 if c.layout == "wide_in" else 0
    g = Guarded.inp(data.to(DT[c.dt]), (2, pad), (3, pad), gpu)
    wide = c.halves or pad
    return g, (g.buf.shape[1] if wide else 0)


class Y:
    """the result buffer of one GroupNorm problem in the case's layout, and what the descriptor needs to write it"""

    def __init__(self, c, imgs, rows, gpu):
        C, R = c.C, imgs * rows
        self.c, self.imgs, self.rows = c, imgs, rows
        self.ldy = self.lo_off = self.y_img_rows = self.y_row0 = 0
        lay = c.layout
        if lay == "wide_out":
            self.ldy = C + 24
            self.g = Guarded.out((1 + R + 2, self.ldy), (slice(1, 1 + R), slice(8, 8 + C)), torch.float16, gpu)
        elif lay == "split":
            self.ldy, self.lo_off = 2 * C + 24, C + 8
            self.g = Guarded.out((1 + R + 2, self.ldy), (slice(1, 1 + R), slice(8, 8 + self.lo_off + C)), torch.float16, gpu)
        elif lay in ("padded0", "padded3"):
            self.y_img_rows, self.y_row0 = rows + 5, int(lay[-1])
            self.g = Guarded.out((1 + imgs * self.y_img_rows + 2, C), (slice(1, 1 + imgs * self.y_img_rows), slice(0, C)), torch.float16, gpu)
        else:
            self.g = Guarded.out((1 + R + 2, C), (slice(1, 1 + R), slice(0, C)), torch.float16, gpu)

    def result(self, what):
        """the [imgs][rows][C] result (hi of a split row), after checking everything no kernel may write"""
        c, C, v = self.c, self.c.C, self.g.view
        self.g.assert_untouched(what)
        if self.lo_off:
            _poison_left(v[:, C:self.lo_off], what + ": the columns between hi and lo")
            return v[:, :C].reshape(self.imgs, self.rows, C)
        if self.y_img_rows:
            v = v.reshape(self.imgs, self.y_img_rows, C)
            _poison_left(v[:, :self.y_row0], what + ": pad rows in front of an image")
            _poison_left(v[:, self.y_row0 + self.rows:], what + ": pad rows behind an image")
            return v[:, self.y_row0:self.y_row0 + self.rows]
        return v.reshape(self.imgs, self.rows, C)

    def lo(self):
        return self.g.view[:, self.lo_off:self.lo_off + self.c.C].reshape(self.imgs, self.rows, self.c.C)


def _split_close(y, ref, bound, what):
    """hi + lo against the fp64 reference: 2^-21 relative plus the statistics term of the bound"""
    both = y.result(what).detach().cpu().double() + y.lo().detach().cpu().double()
    return _close(both, ref, 2.0 ** -21 * ref.abs() + (bound - nf.ulp16(ref)), what + " hi + lo", rounds=False)


def run_gn_case(ops, gpu, c):
    """-> worst |err| / bound over the halves of the case"""
    P = nf.gn_problem(c)
    imgs, rows, C, G = c.imgs, c.rows, c.C, c.G
    gamma, beta = P.gamma.to(gpu), P.beta.to(gpu)
    worst = 0.0
    shards = [(0, nf.shard_rows(rows)), (nf.shard_rows(rows), rows)] if c.layout == "sharded" else [(0, rows)]
    # one input buffer per shard (a rank holds its own frames), both halves inside it
    X = [_x_input(c, P.x[:, a:b].reshape(imgs * (b - a), -1), gpu) for a, b in shards]
    for col0, ref, bound in P.refs:
        what = "%s%s" % (c.name, " half %d" % (col0 // C) if c.halves else "")
        xs = [(g.view[:, col0:col0 + C], ldx) for g, ldx in X]
        sts = [Stats(ops, gpu, imgs, b - a, C, G) for a, b in shards]
        for (xv, ldx), st, (a, b) in zip(xs, sts, shards):
            ops.gn_stats_group([ops.gn_desc(xv, imgs, b - a, C, G, stats=st.view, ldx=ldx)])
            st.check(what + " statistics")
        total = sts[0]
        if len(sts) == 2:                                      # the all-reduce of the frame-sharded plans, in torch
            total = Stats(ops, gpu, imgs, rows, C, G)
            total.view[:imgs * G * 2] = sts[0].sums() + sts[1].sums()
        ys = [Y(c, imgs, b - a, gpu) for a, b in shards]
        for (xv, ldx), y, (a, b) in zip(xs, ys, shards):
            ops.gn_apply_group([ops.gn_desc(xv, imgs, b - a, C, G, stats=total.view, gamma=gamma[col0:col0 + C], beta=beta[col0:col0 + C],
                                            y=y.g.view, eps=nf.EPS, silu=c.silu, ldx=ldx, ldy=y.ldy, lo_off=y.lo_off,
                                            stat_rows=rows if len(shards) == 2 else 0, y_img_rows=y.y_img_rows, y_row0=y.y_row0)])
        torch.cuda.synchronize()
        for g, _ in X:
            g.assert_untouched(what + ": x")
        out = torch.cat([y.result(what) for y in ys], 1)
        worst = max(worst, _close(out, ref, bound, what))
        if c.layout == "split":
            _split_close(ys[0], ref, bound, what)
    return worst


def _run_table(ops, gpu, cases, runner, tag):
    worst, at = 0.0, ""
    STAT_PART[0] = 0.0
    for c in cases:
        r = runner(ops, gpu, c)
        if r > worst:
            worst, at = r, c.name
    print("PARITY %-44s %3d cases, worst err/bound %.3f (%s), statistics term used %.3f" % (tag, len(cases), worst, at, STAT_PART[0]))
    return worst


def _slices(table, n=8):
    """the table in slices of a few cases per test function, so that none runs long"""
    return [table[i:i + n] for i in range(0, len(table), n)]


GN_PLAIN = [c for c in nf.GN if c.kind != "offset"]
GN_OFFSET = [c for c in nf.GN if c.kind == "offset"]


@pytest.mark.parametrize("part", range(len(_slices(GN_PLAIN))))
def test_groupnorm_two_kernel_cases(ops, gpu, part):
    _run_table(ops, gpu, _slices(GN_PLAIN)[part], run_gn_case, "gn_stats + gn_apply [%d]" % part)


def test_groupnorm_two_kernel_offset_cases(ops, gpu):
    """group mean = 32 x its std, fp32 input: the cancellation regime of E[x^2] - mean^2"""
    _run_table(ops, gpu, GN_OFFSET, run_gn_case, "gn_stats + gn_apply, offset kind")


# ------------------------------------------------------------------------------------------------------------------------------------
# ticket reuse and grouped launches of the two-kernel form
# ------------------------------------------------------------------------------------------------------------------------------------
def _sums_reference(x, G):
    s, ss = nf.gn_sums(x.double(), G)
    return torch.stack([s, ss], -1).reshape(-1)


def _sums_close(got, x, G, what):
    """(sum, sum of squares) against fp64: each is a sum of n terms of one sign pattern -> n * 2^-24 * sum |terms| holds for ANY order"""
    ref = _sums_reference(x, G)
    s, ss = nf.gn_sums(x.double().abs(), G)
    mag = torch.stack([s, ss], -1).reshape(-1)
    n = x.shape[1] * (x.shape[2] // G)
    err = (got.detach().cpu().double() - ref).abs()
    assert bool((err <= n * nf.U * mag).all()), (what, float((err / (n * nf.U * mag)).max()))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("imgs,rows,C", [(1, 49, 320), (2, 333, 640), (1, 320, 2048)], ids=["2chunks", "14chunks", "40chunks"])
def test_statistics_buffer_is_reusable(ops, gpu, imgs, rows, C, dt):
    """two launches with different data on ONE statistics buffer: the second meets its own reference, the ticket words read zero after
    each, and a repeat of the first launch is bit-identical to the first"""
    G = 32
    g = torch.Generator().manual_seed(rows + C)
    xa = nf._round(0.5 + torch.randn(imgs, rows, C, generator=g), dt)
    xb = nf._round(-0.25 + 1.5 * torch.randn(imgs, rows, C, generator=g), dt)
    A = Guarded.inp(xa.reshape(imgs * rows, C).to(DT[dt]), (1, 0), (1, 0), gpu)
    B = Guarded.inp(xb.reshape(imgs * rows, C).to(DT[dt]), (1, 0), (1, 0), gpu)
    st = Stats(ops, gpu, imgs, rows, C, G)
    got = []
    for X, x in ((A, xa), (B, xb), (A, xa)):
        ops.gn_stats_group([ops.gn_desc(X.view, imgs, rows, C, G, stats=st.view)])
        st.check("reuse %d x %d x %d" % (imgs, rows, C))
        got.append(st.sums())
        _sums_close(got[-1], x, G, "launch %d" % len(got))
    assert torch.equal(_bits(got[0]), _bits(got[2])) and not torch.equal(got[0], got[1])


def _gn_members(ops, gpu, cases, seed0):
    """per member: its own data (the case's shape, another seed through the name), x, statistics, y and the two descriptors"""
    ms = []
    for i, c in enumerate(cases):
        c = nf.Case({**c, "name": "%s member %d/%d" % (c.name, i, seed0), "seed": i})
        P = nf.gn_problem(c)
        Xg, ldx = _x_input(c, P.x.reshape(c.imgs * c.rows, -1), gpu)
        st, y = Stats(ops, gpu, c.imgs, c.rows, c.C, c.G), Y(c, c.imgs, c.rows, gpu)
        gamma, beta = P.gamma.to(gpu), P.beta.to(gpu)
        d = ops.gn_desc(Xg.view, c.imgs, c.rows, c.C, c.G, stats=st.view, gamma=gamma, beta=beta, y=y.g.view, eps=nf.EPS, silu=c.silu, ldx=ldx)
        ms.append((c, P, Xg, st, y, d, (gamma, beta)))
    return ms


def _base(imgs, rows, C, dt, silu=False):
    return nf.Case(name="group %dx%dx%d %s" % (imgs, rows, C, dt), imgs=imgs, rows=rows, C=C, G=32, dt=dt, kind="plain", silu=silu,
                   stats=nf.mirror_launch_shape(imgs, rows, C, 0), apply=nf.mirror_launch_shape(imgs, rows, C, 1))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_groupnorm_group_is_one_launch_and_bit_identical(ops, gpu, n, dt):
    """n same-shape problems through ctrl_op_gn_stats_group / ctrl_op_gn_apply_group: ONE launch each (the profiler's shape note ends
    in xN) and every member bit for bit what it gets alone"""
    base = _base(2, 333, 640, dt, silu=True)
    prev = ops.set_policy("CTRL_GROUP", "1")
    try:
        single = _gn_members(ops, gpu, [base] * n, 0)
        for m in single:
            ops.gn_stats_group([m[5]])
            ops.gn_apply_group([m[5]])
        grouped = _gn_members(ops, gpu, [base] * n, 0)
        with ops.Profiler() as prof:
            ops.gn_stats_group([m[5] for m in grouped])
            ops.gn_apply_group([m[5] for m in grouped])
        torch.cuda.synchronize()
    finally:
        ops.set_policy("CTRL_GROUP", prev)
    launches = [(r[0], r[2]) for r in prof.launches if r[0].startswith("gn_")]
    assert [l[0] for l in launches] == ["gn_stats", "gn_apply"] and all(l[1].endswith("x%d" % n) for l in launches), launches
    worst = 0.0
    for i, (S, Gm) in enumerate(zip(single, grouped)):
        what = "%s member %d of %d" % (base.name, i, n)
        Gm[3].check(what)
        assert torch.equal(_bits(S[3].sums()), _bits(Gm[3].sums())), what + ": statistics differ from the single launch"
        a, b = S[4].result(what + " single"), Gm[4].result(what + " grouped")
        assert torch.equal(_bits(a), _bits(b)), what + ": result differs from the single launch"
        worst = max(worst, _close(b, Gm[1].refs[0][1], Gm[1].refs[0][2], what))
    assert not torch.equal(grouped[0][4].g.view, grouped[1][4].g.view)           # distinct problems
    print("PARITY gn group of %d %s: one launch per pass, bit-identical, worst err/bound %.3f" % (n, dt, worst))


def test_groupnorm_group_with_unequal_rows_falls_back(ops, gpu):
    cases = [_base(2, 333, 640, "f16"), _base(2, 49, 640, "f16"), _base(2, 333, 640, "f16")]
    ms = _gn_members(ops, gpu, cases, 1)
    with ops.Profiler() as prof:
        ops.gn_stats_group([m[5] for m in ms])
        ops.gn_apply_group([m[5] for m in ms])
    torch.cuda.synchronize()
    launches = [(r[0], r[2]) for r in prof.launches if r[0].startswith("gn_")]
    assert len(launches) == 6 and not any(l[1].endswith(("x2", "x3", "x4")) for l in launches), launches
    for i, m in enumerate(ms):
        what = "mixed group member %d" % i
        m[3].check(what)
        _close(m[4].result(what), m[1].refs[0][1], m[1].refs[0][2], what)


# ------------------------------------------------------------------------------------------------------------------------------------
# gn_fused_kernel
# ------------------------------------------------------------------------------------------------------------------------------------
def _fused_desc(ops, gpu, c, P, y):
    X = Guarded.inp(P.x.reshape(c.imgs * c.rows, c.C).to(DT[c.dt]), (2, 0), (3, 0), gpu)
    gamma, beta = P.gamma.to(gpu), P.beta.to(gpu)
    d = ops.gn_desc(X.view, c.imgs, c.rows, c.C, c.G, gamma=gamma, beta=beta, y=y.g.view, eps=nf.EPS, silu=c.silu, ldy=y.ldy, lo_off=y.lo_off)
    return X, d, (gamma, beta)


def run_fused_case(ops, gpu, c):
    P = nf.gn_problem(c)
    y = Y(c, c.imgs, c.rows, gpu)
    X, d, keep = _fused_desc(ops, gpu, c, P, y)
    ops.gn_fused_group([d])
    torch.cuda.synchronize()
    X.assert_untouched(c.name + ": x")
    r = _close(y.result(c.name), P.refs[0][1], P.refs[0][2], c.name)
    if c.layout == "split":
        _split_close(y, P.refs[0][1], P.refs[0][2], c.name)
    return r


@pytest.mark.parametrize("part", range(len(_slices(nf.FUSED, 10))))
def test_groupnorm_fused_cases(ops, gpu, part):
    _run_table(ops, gpu, _slices(nf.FUSED, 10)[part], run_fused_case, "gn_fused [%d]" % part)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_groupnorm_fused_split_and_wide_output(ops, gpu, dt):
    for C, rows, lay in ((320, 103, "split"), (1280, 409, "split"), (640, 101, "wide_out")):
        c = nf.Case(name="fused %s C%d rows%d %s" % (lay, C, rows, dt), imgs=2, rows=rows, C=C, G=32, dt=dt, kind="spike", silu=True, fused=True,
                    layout=lay)
        print("PARITY %-44s worst err/bound %.3f" % (c.name, run_fused_case(ops, gpu, c)))


@pytest.mark.parametrize("n", [2, 4])
def test_groupnorm_fused_group_is_one_launch_and_bit_identical(ops, gpu, n):
    prev = ops.set_policy("CTRL_GROUP", "1")
    try:
        def members():
            out = []
            for i in range(n):
                c = nf.Case(name="fused group member %d" % i, imgs=2, rows=103, C=640, G=32, dt="f16", kind="plain", silu=True, fused=True, seed=i)
                P = nf.gn_problem(c)
                y = Y(c, c.imgs, c.rows, gpu)
                out.append((c, P, y) + _fused_desc(ops, gpu, c, P, y))
            return out
        single = members()
        for m in single:
            ops.gn_fused_group([m[4]])
        grouped = members()
        with ops.Profiler() as prof:
            ops.gn_fused_group([m[4] for m in grouped])
        torch.cuda.synchronize()
    finally:
        ops.set_policy("CTRL_GROUP", prev)
    launches = [(r[0], r[2]) for r in prof.launches if r[0].startswith("gn_")]
    assert len(launches) == 1 and launches[0][0] == "gn_fused" and launches[0][1].endswith("x%d" % n), launches
    for i, (S, Gm) in enumerate(zip(single, grouped)):
        what = "fused group member %d of %d" % (i, n)
        a, b = S[2].result(what + " single"), Gm[2].result(what + " grouped")
        assert torch.equal(_bits(a), _bits(b)), what
        _close(b, Gm[1].refs[0][1], Gm[1].refs[0][2], what)
    assert not torch.equal(grouped[0][2].g.view, grouped[1][2].g.view)


# ------------------------------------------------------------------------------------------------------------------------------------
# layernorm_kernel
# ------------------------------------------------------------------------------------------------------------------------------------
class LnRun:
    """operands of one LayerNorm case on the device: x (and xsum) at ldx = C + 16 and y at ldy = C + 24 with guard columns on both sides
    and guard rows, or dense between guard rows; addv at ldv = C + 4"""

    def __init__(self, ops, gpu, c):
        P = self.P = nf.ln_problem(c)
        self.c = c
        C, M = c.C, c.M
        px, py = (8, 8) if c.wide else (0, 0)
        self.X = Guarded.inp(P.x.to(DT[c.dt]), (2, px), (3, px), gpu)
        self.Yg = Guarded.out((1 + M + 2, C + 3 * py), (slice(1, 1 + M), slice(py, py + C)), torch.float16, gpu)
        self.ldx, self.ldy = C + 2 * px, C + 3 * py
        self.gamma, self.beta = P.gamma.to(gpu), P.beta.to(gpu)
        self.V = self.S = None
        kw = {}
        if c.add:
            self.V = Guarded.inp(P.addv, (0, 0), (1, 4), gpu)
            self.S = Guarded.out((1 + M + 2, self.ldx), (slice(1, 1 + M), slice(px, px + C)), DT[c.dt], gpu)
            kw = dict(addv=self.V.view, ldv=C + 4, rows_per_img=c.rows_per_img, vmod=c.vmod, xsum=self.S.view)
        self.desc = ops.ln_desc(self.X.view, self.gamma, self.beta, self.Yg.view, M, C, self.ldx, self.ldy, eps=nf.EPS, **kw)

    def check(self):
        c, P = self.c, self.P
        self.X.assert_untouched(c.name + ": x")
        self.Yg.assert_untouched(c.name + ": y")
        if c.add:
            self.V.assert_untouched(c.name + ": addv")
            self.S.assert_untouched(c.name + ": xsum")
            assert torch.equal(_bits(self.S.view), _bits(P.xsum.to(DT[c.dt]))), c.name + ": the stored sum is not x + addv[(row / rows_per_img) % vmod]"
        return _close(self.Yg.view, P.ref, P.bound, c.name)


def run_ln_case(ops, gpu, c):
    R = LnRun(ops, gpu, c)
    if c.add:
        ops.layernorm_add(R.X.view, R.V.view, c.C + 4, c.rows_per_img, c.vmod, R.S.view, R.gamma, R.beta, R.Yg.view, c.M, c.C, R.ldx, R.ldy, eps=nf.EPS)
    else:
        ops.layernorm_group([R.desc])
    torch.cuda.synchronize()
    return R.check()


@pytest.mark.parametrize("nch", [1, 2, 4])
def test_layernorm_cases(ops, gpu, nch):
    _run_table(ops, gpu, [c for c in nf.LN if nf.ln_nch(c.C) == nch], run_ln_case, "layernorm_kernel<%d>" % nch)


def test_layernorm_add_cases(ops, gpu):
    _run_table(ops, gpu, nf.LN_ADD, run_ln_case, "layernorm_kernel + addv")


@pytest.mark.parametrize("add", [False, True], ids=["plain", "addv"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_layernorm_group_is_one_launch_and_bit_identical(ops, gpu, n, add):
    def members():
        return [LnRun(ops, gpu, nf.Case(name="ln group member %d%s" % (i, " add" if add else ""), C=520, M=33, dt=("f16", "f32")[n % 2], wide=True,
                                        add=add or None, rows_per_img=7 if add else None, vmod=3 if add else None, seed=i)) for i in range(n)]
    prev = ops.set_policy("CTRL_GROUP", "1")
    try:
        single = members()
        for R in single:
            ops.layernorm_group([R.desc])
        grouped = members()
        with ops.Profiler() as prof:
            ops.layernorm_group([R.desc for R in grouped])
        torch.cuda.synchronize()
    finally:
        ops.set_policy("CTRL_GROUP", prev)
    launches = [(r[0], r[2]) for r in prof.launches if r[0] == "layernorm"]
    assert len(launches) == 1 and launches[0][1].endswith("x%d" % n), launches
    for S, Gm in zip(single, grouped):
        assert torch.equal(_bits(S.Yg.view), _bits(Gm.Yg.view)), Gm.c.name
        Gm.check()
    assert not torch.equal(grouped[0].Yg.view, grouped[1].Yg.view)


def test_layernorm_mixed_group_falls_back_to_single_launches(ops, gpu):
    """only one member has addv: the members disagree, so three launches -- and every one still right"""
    mk = lambda i, add: LnRun(ops, gpu, nf.Case(name="ln mixed member %d" % i, C=520, M=33, dt="f16", wide=True, add=add or None,
                                                rows_per_img=7 if add else None, vmod=3 if add else None, seed=i))
    ms = [mk(0, False), mk(1, True), mk(2, False)]
    with ops.Profiler() as prof:
        ops.layernorm_group([R.desc for R in ms])
    torch.cuda.synchronize()
    launches = [(r[0], r[2]) for r in prof.launches if r[0] == "layernorm"]
    assert len(launches) == 3 and not any(l[1].endswith(("x2", "x3", "x4")) for l in launches), launches
    for R in ms:
        R.check()
