"""The kernels under the two CLIP towers (csrc/text_gemm.hip, csrc/text.hip, csrc/vision.hip) at their split, tile and row edges, on the
GPU: every case of tests/tower_forms.py through the C entry points against the fp64 references and the element-wise bounds, every
operand inside a guarded allocation (outputs and the split-K workspace poisoned, inputs surrounded by NaN), and the batch invariance of
every family bit for bit.  The checks themselves are tested on the host (tests/test_tower_check_host.py).  Nothing here provokes a
fault: every refused call returns before a launch."""
import ctypes

import pytest
import torch

import helpers
import tower_forms as T
from helpers import Guarded

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
REL_TOL = {F32: 2e-3, F16: 2e-3, BF16: 1e-2}          # the suite's per-tensor tolerances (tests/helpers.py), asserted beside the bounds
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


@pytest.fixture(scope="module")
def L_(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    _lib.lib()
    return _lib


def _close(out, ref, bound, what, family, rel_tol=None):
    """finite, every element within the bound, the per-tensor rel_inf within the suite's tolerance; prints the worst err / bound"""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite outputs" % (what, int((~torch.isfinite(o)).sum()))
    err = (o - ref).abs()
    worst = float((err / bound).max())
    rel = float(err.max() / ref.abs().max().clamp_min(1e-12))
    print("TOWER-WORST %-18s %-58s err/bound %.3f rel_inf %.2e" % (family, what, worst, rel))
    bad = err > bound
    if bool(bad.any()):
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond the bound (worst err/bound %.2f); first at %s: got %.8g want %.8g bound %.3g" % (
            what, int(bad.sum()), bad.numel(), worst, first, float(o[first]), float(ref[first]), float(bound[first])))
    if rel_tol is not None:
        assert rel <= rel_tol, "%s: rel_inf %.3e > %.1e" % (what, rel, rel_tol)
    return worst


def _inp(t, dev, rows=1, cols=0):
    """a 1-D or 2-D input inside NaN: `rows` NaN rows (1-D: 4 * rows elements) before and after, `cols` NaN pad columns (ld = width + cols)"""
    fill = float("nan") if t.is_floating_point() else (255 if t.dtype == torch.uint8 else -(1 << 40))
    if t.dim() == 1:
        return Guarded.inp(t, (4 * rows,), (4 * rows,), dev, fill)
    return Guarded.inp(t, (rows, 0), (rows, cols), dev, fill)


def _out(rows, width, dt, dev, cols=0, pad=1):
    """a [rows][width] output inside poison: `pad` rows before and after, `cols` pad columns"""
    return Guarded.out((rows + 2 * pad, width + cols), (slice(pad, pad + rows), slice(0, width)), dt, dev)


def _untouched(what, *gs):
    for g in gs:
        if g is not None:
            g.assert_untouched(what)


def _p(L_, g):
    return L_.ptr(g.view if isinstance(g, Guarded) else g)


# ---------------------------------------------------------------------------------------------------------------------------
# few-row GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def _run_gemm(L_, dev, N, K, x, act, dt, bias, res):
    """y [M][N] of the rows x [M][K]; returns (y bits on the CPU, guards)"""
    _, W0, b0, _ = T.gemm_operands(N, K)
    M = x.shape[0]
    gx, gW = _inp(x, dev, 2), _inp(W0, dev)
    gb = _inp(b0, dev) if bias else None
    gr = _inp(res, dev) if res is not None else None
    y = _out(M, N, dt, dev)
    n = L_.lib().ctrl_text_gemm_ws_bytes(M, N, K)
    assert n == T.gemm_geometry(N, K)[0] * M * N * 4
    ws = Guarded.out((n // 4 + 8,), (slice(4, 4 + n // 4),), F32, dev)          # exactly ctrl_text_gemm_ws_bytes, poison on both sides
    L_.check(L_.lib().ctrl_op_text_gemm(_p(L_, gx), _p(L_, gW), _p(L_, gb) if bias else None, M, N, K, act, _p(L_, gr) if gr else None,
                                        _p(L_, y), L_.dtype_code(dt), _p(L_, ws), n, L_.cur_stream()))
    torch.cuda.synchronize()
    return y.view.cpu(), (gx, gW, gb, gr, y, ws)


@pytest.mark.parametrize("case_id", [c.id for c in T.GEMM])
def test_text_gemm_case(L_, gpu, case_id):
    c = T.GEMM_BY_ID[case_id]
    x, _, _, r = T.gemm_operands(c.N, c.K)
    y, gs = _run_gemm(L_, gpu, c.N, c.K, x[:c.M], c.act, c.dt, c.bias, r[:c.M] if c.res else None)
    ref, bound = T.gemm_reference(case_id)
    _close(y, ref, bound, case_id, "gemm act%d %s" % (c.act, T.DT_NAME[c.dt]), REL_TOL[c.dt])
    _untouched(case_id, *gs)


@pytest.mark.parametrize("nk", T.GEMM_NK)
def test_text_gemm_rows_do_not_depend_on_the_batch(L_, gpu, nk):
    """the rows of M = 77 are the rows of the M = 33 and M = 65 prefixes bit for bit, and a row permutation of x permutes y: a row's bits
    depend neither on M nor on the row's position"""
    N, K = nk
    x, _, _, r = T.gemm_operands(N, K)
    act = (0, 2, 3)[T.GEMM_NK.index(nk) % 3]
    full, _ = _run_gemm(L_, gpu, N, K, x, act, F32, True, r)
    for M in (33, 65):
        part, _ = _run_gemm(L_, gpu, N, K, x[:M], act, F32, True, r[:M])
        assert torch.equal(helpers._bits(part), helpers._bits(full[:M])), "M = %d prefix differs from the rows inside M = 77" % M
    perm = torch.randperm(T.GEMM_MAXM, generator=torch.Generator().manual_seed(N * K))
    assert not torch.equal(perm, torch.arange(T.GEMM_MAXM))
    moved, _ = _run_gemm(L_, gpu, N, K, x[perm].contiguous(), act, F32, True, r[perm].contiguous())
    assert torch.equal(helpers._bits(moved), helpers._bits(full[perm])), "a row's bits depend on its position"


@pytest.mark.parametrize("case_id", [c.id for c in T.FINISH])
def test_text_gemm_finish_case(L_, gpu, case_id):
    """the finish kernel alone over exact planes: ldres = N + 4, ldy = N + 8; the last case takes the second grid-stride trip"""
    c = T.FIN_BY_ID[case_id]
    p = T.finish_problem(case_id)
    ws = _inp(p["ws"].reshape(-1), gpu)
    gb = _inp(p["bias"], gpu) if c.bias else None
    gr = _inp(p["res"], gpu, 1, 4) if c.res else None
    y = _out(c.M, c.N, c.dt, gpu, cols=8)
    L_.check(L_.lib().ctrl_op_text_gemm_finish(_p(L_, ws), c.splits, c.M, c.N, _p(L_, gb) if gb else None, c.act, _p(L_, gr) if gr else None,
                                               c.N + 4, _p(L_, y), L_.dtype_code(c.dt), c.N + 8, L_.cur_stream()))
    torch.cuda.synchronize()
    _close(y.view, p["ref"], p["bound"], case_id, "finish act%d %s" % (c.act, T.DT_NAME[c.dt]), REL_TOL[c.dt])
    if c.act == 0 and not c.res:          # exact sum, one rounding: the stored value is the rounded reference bit for bit
        assert torch.equal(helpers._bits(y.view), helpers._bits(p["ref"].to(c.dt)))
    _untouched(case_id, ws, gb, gr, y)


def test_text_gemm_refuses_before_it_launches(L_, gpu):
    """an activation or an output type the finish launch would refuse is refused before the partial launch: the workspace stays poisoned"""
    N, K, M = 32, 160, 5
    x, W, _, _ = T.gemm_operands(N, K)
    gx, gW = _inp(x[:M], gpu), _inp(W, gpu)
    y = _out(M, N, F32, gpu)
    n = L_.lib().ctrl_text_gemm_ws_bytes(M, N, K)
    ws = Guarded.out((n // 4 + 8,), (slice(4, 4 + n // 4),), F32, gpu)
    snap = ws.buf.clone()
    for act, dtc, nb in ((1, 0, n), (0, 7, n), (0, 0, n - 4)):
        assert L_.lib().ctrl_op_text_gemm(_p(L_, gx), _p(L_, gW), None, M, N, K, act, None, _p(L_, y), dtc, _p(L_, ws), nb, L_.cur_stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(ws.buf, snap)
    _untouched("refused", y, ws)


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention
# ---------------------------------------------------------------------------------------------------------------------------
def _run_attn(L_, dev, q, k, v, dld=0, dldo=0):
    N, H, L, _ = q.shape
    C = H * 64
    qkv = _inp(T.attn_pack(q, k, v, 3 * C + dld), dev)          # pad columns and the rows before and after: NaN
    out = _out(N * L, C, F16, dev, cols=dldo)
    L_.check(L_.lib().ctrl_op_text_attn(_p(L_, qkv), 3 * C + dld, _p(L_, out), C + dldo, N, L, H, T.ATTN_SCALE, L_.cur_stream()))
    torch.cuda.synchronize()
    return T.attn_unpack(out.view.cpu(), N, H, L), (qkv, out)


@pytest.mark.parametrize("case_id", [c.id for c in T.ATTN])
def test_text_attn_case(L_, gpu, case_id):
    c = T.ATTN_BY_ID[case_id]
    p = T.attn_problem(case_id)
    out, gs = _run_attn(L_, gpu, p["q"], p["k"], p["v"], c.dld, c.dldo)
    w, _ = helpers.assert_attn_close(out, p["ref"], p["bound"], case_id)
    print("TOWER-WORST %-18s %-58s err/bound %.3f" % ("attn " + c.kind, case_id, w))
    # the first token sees itself alone: V[0] rounded to fp16 (it is fp16 already), within the same bound
    r0 = (out[:, :, 0].double() - p["v"][:, :, 0].double()).abs()
    assert bool((r0 <= p["bound"][:, :, 0]).all())
    _untouched(case_id, *gs)


@pytest.mark.parametrize("L", [17, 77, 128])
@pytest.mark.parametrize("kind", ["plain", "diagonal"])
def test_text_attn_prompt_does_not_depend_on_the_batch(L_, gpu, L, kind):
    q1, k1, v1 = T.attn_qkv(kind, L, 1, 3, seed=5)
    qo, ko, vo = T.attn_qkv("plain", L, 2, 3, seed=6)
    alone, _ = _run_attn(L_, gpu, q1, k1, v1)
    for pos in (0, 2):
        cat = lambda a, o: torch.cat([a, o[:1], o[1:]] if pos == 0 else [o[:1], o[1:], a], 0)
        batch, _ = _run_attn(L_, gpu, cat(q1, qo), cat(k1, ko), cat(v1, vo), 8, 16)
        assert torch.equal(helpers._bits(batch[pos]), helpers._bits(alone[0])), "prompt differs at position %d of N = 3" % pos


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------------
ROW_IDS = torch.tensor([[5, 9, 1], [7, 2, 3]], dtype=torch.int64)          # eos = 2 (argmax): prompt 0 pools row 1, prompt 1 row 0
ROW_POOLED = (1, 0)


def _ln_check(out, x, g, b, dt, kind, what, family):
    ref, bound = T.ln_ref(x, g, b, dt, kind)
    if kind == "flat":
        want = b.to(dt).expand(x.shape[0], -1)
        assert torch.equal(helpers._bits(out), helpers._bits(want)), "%s: a flat row must give beta bit for bit" % what
    if kind != "flat":          # the share of the statistics term in use, the rounding of the output taken off (tests/tower_forms.py)
        print("TOWER-SHARE %-18s %-58s statistics share %.3f" % (family, what, T.ln_stat_share(out, x, g, b, dt, kind)))
    return _close(out, ref, bound, what, family, 1e-2 if dt == BF16 else 2e-3)


def _text_embed(L_, dev, ids, tok, pos, g, b, bad=None):
    N, L = ids.shape
    C = tok.shape[1]
    gi, gt, gp, gg, gb = _inp(ids.reshape(-1), dev), _inp(tok, dev), _inp(pos, dev), _inp(g, dev), _inp(b, dev)
    x, y = _out(N * L, C, F32, dev), _out(N * L, C, F16, dev)
    L_.check(L_.lib().ctrl_op_text_embed(_p(L_, gi), _p(L_, gt), _p(L_, gp), tok.shape[0], N, L, C, _p(L_, x), _p(L_, gg), _p(L_, gb), T.EPS,
                                         _p(L_, y), L_.ptr(bad), L_.cur_stream()))
    torch.cuda.synchronize()
    return x.view.cpu(), y.view.cpu(), (gi, gt, gp, gg, gb, x, y)


def _embed_tables(kind, V, L, C):
    tok, g, b = T.row_data(kind, V, C, "tok")
    if kind == "flat":
        return torch.full((V, C), 1.0), torch.full((L, C), 0.5), g, b
    return tok, 0.1 * torch.randn(L, C, generator=T._gen("pos", L, C)), g, b


def _text_final(L_, dev, x, xdt, g, b, ydt, ids, eos, want_y=True, want_pooled=True, ext=False):
    """returns (y, pooled, pooled32, guards); ids [N][L]"""
    rows, C = x.shape
    N, L = ids.shape
    gx, gg, gb, gi = _inp(x.to(xdt), dev), _inp(g, dev), _inp(b, dev), _inp(ids.reshape(-1), dev)
    y = _out(rows, C, ydt, dev) if want_y else None
    pooled = _out(N, C, ydt, dev) if want_pooled else None
    p32 = _out(N, C, F32, dev) if ext else None
    args = [_p(L_, gx), L_.dtype_code(xdt), rows, C, _p(L_, gg), _p(L_, gb), T.EPS, _p(L_, y) if y else None, L_.dtype_code(ydt), _p(L_, gi), L,
            eos, _p(L_, pooled) if pooled else None]
    if ext:
        L_.check(L_.lib().ctrl_op_text_final_ln_ext(*args, _p(L_, p32), L_.cur_stream()))
    else:
        L_.check(L_.lib().ctrl_op_text_final_ln(*args, L_.cur_stream()))
    torch.cuda.synchronize()
    cpu = lambda t: t.view.cpu() if t is not None else None
    return cpu(y), cpu(pooled), cpu(p32), (gx, gg, gb, gi, y, pooled, p32)


def _vision_embed(L_, dev, patch, cls, pos, g0, b0, g1, b1, N, L):
    C = cls.shape[0]
    gs = [_inp(t, dev) for t in (patch, cls, pos, g0, b0, g1, b1)]
    x, y = _out(N * L, C, F32, dev), _out(N * L, C, F16, dev)
    L_.check(L_.lib().ctrl_op_vision_embed(*[_p(L_, t) for t in gs[:3]], N, L, C, *[_p(L_, t) for t in gs[3:]], T.EPS, _p(L_, x), _p(L_, y),
                                           L_.cur_stream()))
    torch.cuda.synchronize()
    return x.view.cpu(), y.view.cpu(), gs + [x, y]


def _vision_cls(L_, dev, x0, g, b, ydt, outs, L=3):
    """x0 [N][C]: row 0 of every image; every other row of x is NaN (it is never read)"""
    N, C = x0.shape
    x = torch.full((N * L, C), float("nan"))
    x[::L] = x0
    gx, gg, gb = _inp(x, dev), _inp(g, dev), _inp(b, dev)
    pooled = _out(N, C, ydt, dev) if outs in ("both", "pooled") else None
    p32 = _out(N, C, F32, dev) if outs in ("both", "pooled32") else None
    L_.check(L_.lib().ctrl_op_vision_cls_ln(_p(L_, gx), N, L, C, _p(L_, gg), _p(L_, gb), T.EPS, _p(L_, pooled) if pooled else None,
                                            L_.dtype_code(ydt), _p(L_, p32) if p32 else None, L_.cur_stream()))
    torch.cuda.synchronize()
    cpu = lambda t: t.view.cpu() if t is not None else None
    return cpu(pooled), cpu(p32), (gx, gg, gb, pooled, p32)


@pytest.mark.parametrize("case_id", [c.id for c in T.ROWS])
def test_row_kernel_case(L_, gpu, case_id):
    c = T.ROW_BY_ID[case_id]
    C, kind = c.C, c.kind
    N, L = T.ROW_N, T.ROW_L
    if c.op == "text_embed":
        V = 5
        ids = torch.tensor([[0, 4, 2], [3, 3, 1]], dtype=torch.int64)
        tok, pos, g, b = _embed_tables(kind, V, L, C)
        x, y, gs = _text_embed(L_, gpu, ids, tok, pos, g, b)
        want = tok[ids.reshape(-1)] + pos.repeat(N, 1)
        assert torch.equal(helpers._bits(x), helpers._bits(want)), "the stream is tok[id] + pos[l], one fp32 add"
        _ln_check(y, want, g, b, F16, kind, case_id, "row " + kind)
    elif c.op in ("text_final", "text_final_ext"):
        ext = c.op == "text_final_ext"
        x, g, b = T.row_data(kind, N * L, C, c.op)
        x = x.to(c.xdt).float()
        y, pooled, p32, gs = _text_final(L_, gpu, x, c.xdt, g, b, c.ydt, ROW_IDS, 2, want_y=not c.y_null, ext=ext)
        rows = [n * L + ROW_POOLED[n] for n in range(N)]
        if y is not None:
            _ln_check(y, x, g, b, c.ydt, kind, case_id, "row " + kind)
            assert torch.equal(helpers._bits(pooled), helpers._bits(y[rows])), "the pooled row is the row of y"
        else:
            _ln_check(pooled, x[rows], g, b, c.ydt, kind, case_id, "row " + kind)
        if ext:
            _ln_check(p32, x[rows], g, b, F32, kind, case_id + " pooled32", "row " + kind)
            assert torch.equal(helpers._bits(pooled), helpers._bits(p32.to(c.ydt))), "pooled is pooled32 rounded to the output type"
    elif c.op == "vision_embed":
        Lv = c.L
        e, g0, b0 = T.row_data(kind, 1 + N * (Lv - 1), C, "ve")
        _, g1, b1 = T.row_data("plain", 1, C, "ve1")
        if kind == "flat":
            cls, patch, pos = torch.full((C,), 1.0), torch.full((N * (Lv - 1), C), 1.0), torch.full((Lv, C), 0.5)
        else:
            cls, patch, pos = e[0].clone(), e[1:].clone(), 0.1 * torch.randn(Lv, C, generator=T._gen("vpos", Lv, C))
        x, y, gs = _vision_embed(L_, gpu, patch, cls, pos, g0, b0, g1, b1, N, Lv)
        emb = torch.cat([cls.view(1, 1, C).expand(N, 1, C), patch.view(N, Lv - 1, C)], 1) + pos[None]
        _ln_check(x, emb.reshape(N * Lv, C), g0, b0, F32, kind, case_id + " x", "row " + kind)
        assert torch.equal(helpers._bits(x[0]), helpers._bits(x[Lv])), "the class row is shared between the images"
        # layer_norm1 of the stream as it was stored: the kernel normalises exactly those fp32 values
        _ln_check(y, x, g1, b1, F16, "plain", case_id + " y", "row plain")
    else:
        x0, g, b = T.row_data(kind, N, C, "cls")
        pooled, p32, gs = _vision_cls(L_, gpu, x0, g, b, c.ydt, c.outs)
        if pooled is not None:
            _ln_check(pooled, x0, g, b, c.ydt, kind, case_id, "row " + kind)
        if p32 is not None:
            _ln_check(p32, x0, g, b, F32, kind, case_id + " pooled32", "row " + kind)
        if pooled is not None and p32 is not None:
            assert torch.equal(helpers._bits(pooled), helpers._bits(p32.to(c.ydt)))
    _untouched(case_id, *gs)


@pytest.mark.parametrize("C", [257, 1280])
def test_row_kernels_do_not_depend_on_the_batch(L_, gpu, C):
    """one prompt (image) alone, as prompt 0 and as prompt 2 of N = 3: the same bits from every row kernel"""
    L, V = 3, 6
    tok, pos, g, b = _embed_tables("plain", V, L, C)
    ids1 = torch.tensor([[4, 1, 5]], dtype=torch.int64)
    other = torch.tensor([[0, 2, 3], [5, 5, 0]], dtype=torch.int64)
    x1, g1, b1 = T.row_data("plain", L, C, "inv")
    xo, _, _ = T.row_data("offset", 2 * L, C, "inv-other")
    patch1, patcho = x1[:L - 1], xo[:2 * (L - 1)]
    ex, ey, _ = _text_embed(L_, gpu, ids1, tok, pos, g, b)
    fy, fp, f32_, _ = _text_final(L_, gpu, x1, F32, g1, b1, F16, ids1, 2, ext=True)
    vx, vy, _ = _vision_embed(L_, gpu, patch1, tok[0], pos, g, b, g1, b1, 1, L)
    cp, c32, _ = _vision_cls(L_, gpu, x1[:1], g1, b1, BF16, "both")
    for posn in (0, 2):
        put = lambda a, o: torch.cat([a, o] if posn == 0 else [o, a], 0)
        ids3 = put(ids1, other)
        sl = slice(posn * L, posn * L + L)
        bx, by, _ = _text_embed(L_, gpu, ids3, tok, pos, g, b)
        assert torch.equal(bx[sl], ex) and torch.equal(by[sl], ey), "text_embed at position %d" % posn
        gy, gp, g32, _ = _text_final(L_, gpu, put(x1, xo), F32, g1, b1, F16, ids3, 2, ext=True)
        assert torch.equal(gy[sl], fy) and torch.equal(gp[posn], fp[0]) and torch.equal(g32[posn], f32_[0]), "text_final at position %d" % posn
        wx, wy, _ = _vision_embed(L_, gpu, put(patch1, patcho), tok[0], pos, g, b, g1, b1, 3, L)
        assert torch.equal(wx[sl], vx) and torch.equal(wy[sl], vy), "vision_embed at position %d" % posn
        dp, d32, _ = _vision_cls(L_, gpu, put(x1[:1], xo[:2]), g1, b1, BF16, "both")
        assert torch.equal(helpers._bits(dp[posn]), helpers._bits(cp[0])) and torch.equal(d32[posn], c32[0]), "vision_cls_ln at position %d" % posn


@pytest.mark.parametrize("L", T.POOL_LS)
@pytest.mark.parametrize("ext", [False, True])
def test_pooled_index_placements(L_, gpu, L, ext):
    """every placement of tests/tower_forms.py: pool_table(L), one prompt each, batched per rule: the pooled row is the row of an fp32 y bit
    for bit, pooled32 is pooled, and nothing but the prompts' rows is written"""
    C = 64
    table = T.pool_table(L)
    for eos in (2, T.POOL_EOS):
        rows = [r for r in table if r[1] == eos]
        ids = torch.tensor([r[2] for r in rows], dtype=torch.int64)
        N = len(rows)
        x, g, b = T.row_data("plain", N * L, C, "pool", L)
        y, pooled, p32, gs = _text_final(L_, gpu, x, F32, g, b, F32, ids, eos, ext=ext)
        for n, (name, _, _, want) in enumerate(rows):
            assert torch.equal(pooled[n], y[n * L + want]), "L = %d, %s: prompt %d did not pool row %d" % (L, name, n, want)
        if ext:
            assert torch.equal(pooled, p32)
        _untouched("pooled index L = %d" % L, *gs)


def test_text_embed_clamps_ids_and_raises_the_flag(L_, gpu):
    V, L, C = 5, 4, 257
    tok, pos, g, b = _embed_tables("plain", V, L, C)
    good = torch.tensor([[0, 4, 2, 1]], dtype=torch.int64)
    bad_ids = torch.tensor([[-1, V, 2, 1 << 40]], dtype=torch.int64)
    clamped = torch.tensor([[0, V - 1, 2, V - 1]], dtype=torch.int64)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    x0, y0, gs0 = _text_embed(L_, gpu, good, tok, pos, g, b, flag)
    assert int(flag.item()) == 0
    xc, yc, _ = _text_embed(L_, gpu, clamped, tok, pos, g, b, flag)
    assert int(flag.item()) == 0
    x1, y1, gs1 = _text_embed(L_, gpu, bad_ids, tok, pos, g, b, flag)
    assert int(flag.item()) == 1
    assert torch.equal(x1, xc) and torch.equal(y1, yc), "id -1 reads row 0, ids >= V read row V - 1"
    x2, y2, gs2 = _text_embed(L_, gpu, bad_ids, tok, pos, g, b, None)          # no flag word: accepted
    assert torch.equal(x2, xc) and torch.equal(y2, yc)
    _untouched("id clamp", *(gs0 + gs1 + gs2))


# ---------------------------------------------------------------------------------------------------------------------------
# text_proj, text_store, vision_vt, vision_patchify, clip_resize_aa
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.PROJ, ids=[c.id for c in T.PROJ])
def test_text_proj_case(L_, gpu, c):
    a, w, ref, bound = T.proj_problem(c)
    ga, gw = _inp(a, gpu), _inp(w, gpu)
    out = _out(c.N, c.P, c.dt, gpu)
    L_.check(L_.lib().ctrl_op_text_proj(_p(L_, ga), _p(L_, gw), c.N, c.C, c.P, _p(L_, out), L_.dtype_code(c.dt), L_.cur_stream()))
    torch.cuda.synchronize()
    _close(out.view, ref, bound, c.id, "proj " + T.DT_NAME[c.dt], REL_TOL[c.dt])
    if c.N == 3:          # a prompt's projection depends on its own row alone
        one = _out(1, c.P, c.dt, gpu)
        g1 = _inp(a[2:3], gpu)
        L_.check(L_.lib().ctrl_op_text_proj(_p(L_, g1), _p(L_, gw), 1, c.C, c.P, _p(L_, one), L_.dtype_code(c.dt), L_.cur_stream()))
        torch.cuda.synchronize()
        assert torch.equal(helpers._bits(one.view), helpers._bits(out.view[2:3]))
    _untouched(c.id, ga, gw, out)


@pytest.mark.parametrize("n", T.STORE_NS)
@pytest.mark.parametrize("dt", T.DTYPES, ids=["f32", "f16", "bf16"])
def test_text_store_is_the_torch_cast(L_, gpu, n, dt):
    x = torch.randn(n, generator=T._gen("store", n)) * 3.0
    gx = _inp(x, gpu)
    y = Guarded.out((n + 16,), (slice(8, 8 + n),), dt, gpu)
    L_.check(L_.lib().ctrl_op_text_store(_p(L_, gx), _p(L_, y), L_.dtype_code(dt), n, L_.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(helpers._bits(y.view), helpers._bits(x.to(dt)))
    _untouched("store", gx, y)


@pytest.mark.parametrize("c", T.VT, ids=[c.id for c in T.VT])
def test_vision_vt_case(L_, gpu, c):
    """the transpose bit for bit and every pad column exactly zero -- for image 0 of N = 2 the rows after L are image 1's, for the last
    image they are the NaN rows that follow the buffer"""
    v = torch.randn(c.N * c.L, c.C, generator=T._gen("vt", c.id)).half()
    if c.qkv:          # V at column 2 C of a Q | K | V buffer, as the plan passes it
        qkv = torch.randn(c.N * c.L, 3 * c.C, generator=T._gen("vtq", c.id)).half()
        qkv[:, 2 * c.C:] = v
        gv = _inp(qkv, gpu, rows=c.Lkpad)
        vptr, ld = gv.view[:, 2 * c.C:], 3 * c.C
    else:
        gv = _inp(v, gpu, rows=c.Lkpad)
        vptr, ld = gv.view, c.C
    vt = Guarded.out((c.N * c.C + 2, c.Lkpad), (slice(1, 1 + c.N * c.C), slice(0, c.Lkpad)), F16, gpu)
    L_.check(L_.lib().ctrl_op_vision_vt(L_.ptr(vptr), ld, _p(L_, vt), c.N, c.L, c.C, c.Lkpad, L_.cur_stream()))
    torch.cuda.synchronize()
    got = vt.view.cpu().reshape(c.N, c.C, c.Lkpad)
    assert bool((helpers._bits(got[:, :, c.L:]) == 0).all()), "a pad column is not +0"
    assert torch.equal(helpers._bits(got), helpers._bits(T.vt_expected(v, c.N, c.L, c.C, c.Lkpad)))
    _untouched(c.id, gv, vt)


def _ms():
    return (ctypes.c_float * 6)(*(MEAN + STD))


@pytest.mark.parametrize("c", T.PATCH, ids=[c.id for c in T.PATCH])
def test_vision_patchify_case(L_, gpu, c):
    from test_gpu_vision_encoder import _im2col
    N, S, p = 2, c.S, c.p
    g = T._gen("patch", c.id)
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    if c.kind == "u8_norm":
        u8 = torch.randint(0, 256, (N, S, S, 3), generator=g, dtype=torch.uint8)
        src, dt = u8, L_.U8_NHWC
        want = ((u8.permute(0, 3, 1, 2).float() / 255.0 - m) / s).half()
    else:
        tdt = {"f32_norm": F32, "f16_plain": F16, "bf16_norm": BF16}[c.kind]
        src = torch.rand(N, 3, S, S, generator=g).to(tdt)
        dt = L_.dtype_code(tdt)
        want = src.half() if c.kind == "f16_plain" else ((src.float() - m) / s).half()
    cols = _im2col(want, p)
    cols = torch.nn.functional.pad(cols, (0, c.Kpad - cols.shape[1]))
    gsrc = _inp(src.reshape(-1), gpu)
    out = _out(N * (S // p) ** 2, c.Kpad, F16, gpu)
    L_.check(L_.lib().ctrl_op_vision_patchify(_p(L_, gsrc), dt, N, S, p, None if c.kind == "f16_plain" else _ms(), _p(L_, out), c.Kpad,
                                              L_.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(helpers._bits(out.view), helpers._bits(cols))
    _untouched(c.id, gsrc, out)


def _resize(L_, dev, src, dtc, N, H, W, OH, OW, norm, out_dt):
    gsrc = _inp(src.reshape(-1), dev)
    out = Guarded.out((N * 3 * OH * OW + 16,), (slice(8, 8 + N * 3 * OH * OW),), out_dt, dev)
    L_.check(L_.lib().ctrl_op_clip_resize_aa(_p(L_, gsrc), dtc, N, H, W, OH, OW, _ms() if norm else None, _p(L_, out), L_.dtype_code(out_dt),
                                             L_.cur_stream()))
    torch.cuda.synchronize()
    _untouched("resize", gsrc, out)
    return out.view.cpu().reshape(N, 3, OH, OW)


@pytest.mark.parametrize("c", T.RESIZE, ids=[c.id for c in T.RESIZE])
def test_clip_resize_aa_case(L_, gpu, c):
    from clip_vision_ref import resize_with_antialiasing
    H, W, OH, OW = c.size
    N = 2
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=T._gen("resize", c.size), dtype=torch.uint8)
    x01 = u8.float().div(255.0).permute(0, 3, 1, 2).contiguous()
    if c.src == "u8":
        out = _resize(L_, gpu, u8, L_.U8_NHWC, N, H, W, OH, OW, c.norm, c.out)
        same = _resize(L_, gpu, x01, L_.dtype_code(F32), N, H, W, OH, OW, c.norm, c.out)
        assert torch.equal(helpers._bits(out), helpers._bits(same)), "uint8 and fp32 inputs of one image differ"
    else:
        x01 = x01 if c.src == "f32" else x01.half()
        out = _resize(L_, gpu, x01, L_.dtype_code(x01.dtype), N, H, W, OH, OW, c.norm, c.out)
    ref = (resize_with_antialiasing(x01.float() * 2.0 - 1.0, (OH, OW)) + 1.0) / 2.0
    if c.norm:
        ref = (ref - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    ref = ref.double()
    _close(out, ref, T.resize_tol(ref, c.out, STD if c.norm else None), c.id, "resize " + T.DT_NAME[c.out])


def test_clip_resize_aa_refuses_65_taps(L_, gpu):
    H, W, OH, OW = T.RESIZE_REFUSED
    src = _inp(torch.rand(3 * H * W), gpu)
    out = Guarded.out((3 * OH * OW + 16,), (slice(8, 8 + 3 * OH * OW),), F32, gpu)
    snap = out.buf.clone()
    assert L_.lib().ctrl_op_clip_resize_aa(_p(L_, src), 0, 1, H, W, OH, OW, None, _p(L_, out), 0, L_.cur_stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(out.buf, snap)
