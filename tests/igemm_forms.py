"""The pure-data part of tests/test_gpu_igemm_forms.py: the table of kernel forms (FORMS, SPLITK), the edge-case generators, and the
construction of a case's operands and descriptor on a given device.  The GPU test launches every case; tests/test_igemm_select_host.py
asks the selector (ctrl_igemm_select) about every case over CPU tensors of the same shapes, paddings and alignments."""
import contextlib
import types

import torch
import torch.nn.functional as F

from helpers import Guarded

ROWS, CONV, TEMP = 0, 1, 2
F16, F32, BF16 = torch.float16, torch.float32, torch.bfloat16


def ring(bm, bn, bk, wm, wn, ns, mode, swap=True):
    return "igemm_kernel<%d, %d, %d, %d, %d, %d, %d, %s>" % (bm, bn, bk, wm, wn, ns, mode, "true" if swap else "false")


def wide8(ni, mode):
    return "igemm8_kernel<%d, %d>" % (ni, mode)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(shape, g, scale=1.0):
    """fp16-representable fp32 values (g = None: unset values of that shape)"""
    if g is None:
        return torch.empty(*shape)
    return (torch.randn(*shape, generator=g) * scale).half().float()


class Case(dict):
    __getattr__ = dict.get


def C(name, **kw):
    return Case(name=name, **kw)


def _conv_geom(c):
    up, st = c.up or 1, c.stride or 1
    taps = c.taps or 9
    if taps == 1:
        Ho, Wo = (c.H * up - 1) // st + 1, (c.W * up - 1) // st + 1
    elif c.tap_origin:
        Ho, Wo = (c.H * up + 1 - 3) // st + 1, (c.W * up + 1 - 3) // st + 1          # F.pad(x, (0, 1, 0, 1)), then padding 0
    else:
        Ho, Wo = (c.H * up + 2 - 3) // st + 1, (c.W * up + 2 - 3) // st + 1
    return taps, st, up, Ho, Wo


def _contract(c, a, w):
    """fp64 A . W^T of the case's gather: a = the logical activations (fp64), w = logical weights (fp64); returns [M][Nout]"""
    if c.mode == ROWS:
        return a @ w.t()
    if c.mode == CONV:
        taps, st, up, Ho, Wo = _conv_geom(c)
        x = a.permute(0, 3, 1, 2)
        if up == 2:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        if taps == 9 and c.tap_origin:
            y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=st)
        else:
            y = F.conv2d(x, w, stride=st, padding=1 if taps == 9 else 0)
        assert y.shape[2] == Ho and y.shape[3] == Wo, (y.shape, Ho, Wo)
        return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    # temporal: a = [b][F (+2 with t_pad)][HW][Cin], w = [Nout][Cin][3]
    xp = a if c.t_pad else F.pad(a, (0, 0, 0, 0, 1, 1))
    Fr = xp.shape[1] - 2
    y = sum(xp[:, t:t + Fr] @ w[:, :, t].t() for t in range(3))
    return y.reshape(-1, w.shape[0])


def make_problem(ops, device, c, seed=0, reference=True):
    """the operands of case `c` inside poisoned surroundings on `device`, the ops.igemm keyword arguments over them (.kw) and the fp64
    reference.  reference=False: the values stay unset and no reference is computed -- what the selector looks at (shapes, strides,
    paddings, pointer alignments) is the same"""
    g = _gen(1000 + seed) if reference else None     # (no generator: _h and rnd leave the values unset)
    rnd = (lambda *shape: torch.randn(*shape, generator=g)) if reference else torch.empty
    mode, Cin, Nout = c.mode, c.Cin, c.Nout
    odt = c.out or F16
    a_split = c.a_split or 0
    Cl = Cin // 2 if a_split else Cin                 # logical channels (split operand: A rows are [hi | lo])
    # ---- operands ----
    if mode == ROWS:
        taps, M = 1, c.M
        a_log = rnd(M, Cl) if a_split else _h((M, Cl), g)
        w_log = _h((Nout, Cl), g, 0.05)
        w_pack = w_log
        rpi = c.rpi or 24
        geom = None
    elif mode == CONV:
        taps, st, up, Ho, Wo = _conv_geom(c)
        M = c.n * Ho * Wo
        a_log = rnd(c.n, c.H, c.W, Cl) if a_split else _h((c.n, c.H, c.W, Cl), g)
        k = 3 if taps == 9 else 1
        w_log = _h((Nout, Cl, k, k), g, 0.05)
        w_pack = w_log.permute(0, 2, 3, 1).reshape(Nout, taps * Cl)
        rpi = Ho * Wo
        geom = dict(Hin=c.H, Win=c.W, Hout=Ho, Wout=Wo, stride=st, up=up)
    else:
        taps = 3
        M = c.b * c.F * c.HW
        a_log = _h((c.b, c.F + (2 if c.t_pad else 0), c.HW, Cl), g)
        w_log = _h((Nout, Cl, 3), g, 0.05)
        w_pack = w_log.permute(0, 2, 1).reshape(Nout, 3 * Cl)
        rpi = c.rpi or c.HW
        geom = None
    if a_split:
        hi = a_log.half()
        lo = (a_log - hi.float()).half()
        a_dev = torch.cat([hi, lo], dim=-1)
        a_val = hi.double() + lo.double()              # what the kernel multiplies (exactly)
        a_abs = hi.double().abs() + lo.double().abs()
    else:
        a_dev = a_log.half()
        a_val = a_log.double()
        a_abs = a_val.abs()
    Ktot = taps * Cin
    nimg = (M + rpi - 1) // rpi
    bias = rnd(Nout)
    rowvec = rnd(nimg, Nout)
    res = None
    if c.res is not None:
        if c.res_up == 2:
            rshape = (c.n, Ho // 2, Wo // 2, Nout)
        else:
            rshape = (M, Nout)
        res = rnd(*rshape)                              # fp32: NOT fp16-representable
        if c.res == F16:
            res = res.half().float()
    scale = 1.0 if c.scale is None else c.scale
    # ---- fp64 reference and magnitude ----
    ref = mag = None
    colscale = torch.full((Nout,), float(scale), dtype=torch.float64)
    if c.scale2_from:
        colscale[c.scale2_from:(c.scale2_to or Nout)] = c.scale2
    if reference:
        lin = _contract(c, a_val, w_log.double())
        mag = _contract(c, a_abs, w_log.double().abs())
        img = torch.arange(M) // rpi
        add = bias.double()[None, :] + rowvec.double()[img]
        madd = bias.double().abs()[None, :] + rowvec.double().abs()[img]
        if res is not None:
            r2 = res.double()
            if c.res_up == 2:
                r2 = r2.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            r2 = r2.reshape(M, Nout)
            add = add + r2
            madd = madd + r2.abs()
        ref = (lin + add) * colscale[None, :]
        mag = mag + madd
    # ---- device buffers inside poisoned surroundings ----
    nd = a_dev.dim()
    if mode == ROWS:
        A = Guarded.inp(a_dev, (0, 0), (256, 8), device)
    else:
        A = Guarded.inp(a_dev, (1,) + (0,) * (nd - 1), (1,) + (0,) * (nd - 2) + (8,), device)
    lda = Cin + 8
    Wg = Guarded.inp(w_pack.half().contiguous(), (0, 0), (64, 0), device)
    Bg = Guarded.inp(bias, (0,), (64,), device)
    Rv = Guarded.inp(rowvec, (0, 0), (2, 0), device)
    Rs, ldres = None, 0
    if res is not None:
        rd = res.to(c.res)
        Rs = Guarded.inp(rd, (0,) * rd.dim(), (64,) + (0,) * (rd.dim() - 2) + (8,), device) if rd.dim() == 2 else \
            Guarded.inp(rd, (0,) * rd.dim(), (1,) + (0,) * (rd.dim() - 2) + (8,), device)
        ldres = Nout + 8
    pad = 16 if c.pad is None else c.pad
    Lt = c.L or 0
    if Lt:                                             # one transposed segment: [img][Nout][L + pad], one guard image beyond the batch
        Bt = M // Lt
        assert Bt * Lt == M
        O = Guarded.out((Bt + 1, Nout, Lt + pad), (slice(0, Bt), slice(0, Nout), slice(0, Lt)), odt, device)
        segs = [(O.view, Lt + pad, 0, Nout, ops.SEG_TRANSPOSED, Lt)]
    else:
        O = Guarded.out((M + 64, Nout + pad), (slice(0, M), slice(0, Nout)), odt, device)
        segs = [(O.view, Nout + pad, 0, Nout, ops.SEG_ROW, 1)]
    Mir, ld16, lo_off = None, 0, 0
    if c.mirror:
        if c.mirror == "split":
            ld16, lo_off = 2 * Nout + 16, Nout
            Mir = Guarded.out((M + 64, ld16), (slice(0, M), slice(0, 2 * Nout)), F16, device)
        else:
            ld16 = Nout + 16
            Mir = Guarded.out((M + 64, ld16), (slice(0, M), slice(0, Nout)), F16, device)
    kw = dict(A=A.view, lda=lda, W=Wg.view, M=M, Nout=Nout, Cin=Cin, taps=taps, mode=mode, geom=geom, bias=Bg.view, rowvec=Rv.view,
              rows_per_img=rpi, res=Rs.view if Rs else None, ldres=ldres, scale=scale, segs=segs, F=c.F or 0, HW=c.HW or 0,
              out16=Mir.view if Mir else None, ld16=ld16, out16_lo_off=lo_off, a_split=a_split, t_pad=bool(c.t_pad),
              scale2=c.scale2 or 0.0, scale2_from=c.scale2_from or 0, scale2_to=c.scale2_to or 0, res_up=c.res_up or 0,
              tap_origin=c.tap_origin or 0)
    return types.SimpleNamespace(kw=kw, A=A, Wg=Wg, Bg=Bg, Rv=Rv, Rs=Rs, O=O, Mir=Mir, Ws=None, Tk=None, sk=1, twords=0, M=M, Nout=Nout, Ktot=Ktot, Lt=Lt,
                                 lo_off=lo_off, ref=ref, mag=mag, colscale=colscale)


@contextlib.contextmanager
def case_policy(ops, c):
    """the case's policy overrides and `wide` setting, restored on the way out"""
    prev = {}
    try:
        for name, val in (c.policy or {}).items():
            prev[name] = ops.set_policy(name, val)
        if c.wide is not None:
            ops.set_igemm_wide(c.wide)
        yield
    finally:
        if c.wide is not None:
            ops.set_igemm_wide(-1)
        for name, val in prev.items():
            ops.set_policy(name, val)


def attach_splitk(ops, device, c, P):
    """scratch and ticket words of a split-K case, sized exactly by the library with a guard page after each (inside case_policy: the
    split count depends on set_igemm_wide)"""
    probe = torch.zeros(64, dtype=torch.float32, device=device)          # (the split choice depends on the descriptor, not on the scratch)
    P.sk, ws_bytes, P.twords = ops.igemm_splitk_plan(ops.igemm_desc(splitk_ws=probe, **P.kw))
    assert P.sk == c.sk, "%s: the library would use %d K splits, the table says %d" % (c.name, P.sk, c.sk)
    assert ws_bytes % 4 == 0
    P.Ws = Guarded.out((ws_bytes // 4 + 1024,), (slice(0, ws_bytes // 4),), F32, device)
    P.kw["splitk_ws"] = P.Ws.view
    if c.tickets:
        assert P.twords > 0
        P.Tk = Guarded.inp(torch.zeros(P.twords, dtype=torch.int32), (0,), (1024,), device, fill=0x5A5A5A5A)
        P.kw["splitk_tickets"] = P.Tk.view


# ------------------------------------------------------------------------------------------------------------------------------------
# edge generators
# ------------------------------------------------------------------------------------------------------------------------------------
def rows_edges(tag, bm, bn, bk, nstage, scalar=False, m_base=0, policy=None, wide=None, extra=None, ktiles=None, pinned=False, nouts=None, k_m=None):
    """IG_ROWS edge cases of one form: M in {1, BM-1, BM, BM+1, 2 BM + 37} (offset by m_base whole tiles where the form needs a
    filled grid), Nout in {BN, BN + 16, BN + 8 (scalar epilogue)}, k-tiles in {1, 2, NSTAGE - 1, NSTAGE, NSTAGE + 1, 11}"""
    out = []
    extra = extra or {}
    pad = 12 if scalar == "ld" else 16                 # ld % 8 != 0 sends an aligned Nout to the scalar epilogue
    kts = ktiles or sorted({1, 2, nstage - 1, nstage, nstage + 1, 11})
    base = dict(mode=ROWS, policy=policy, wide=wide, pad=pad, pinned=pinned, **extra)
    nouts = nouts or ([bn + 8, bn + 24] if scalar == "n" else [bn, bn + 16])
    k_m = k_m or nstage + 1
    ms = [1, bm - 1, bm, bm + 1, 2 * bm + 37]
    for i, m in enumerate(ms):
        out.append(C("%s M%d" % (tag, m_base + m), M=m_base + m, Nout=nouts[i % len(nouts)], Cin=bk * k_m, res=(F16, F32)[i % 2],
                     out=(F16, F32, BF16)[i % 3], scale=(1.0, 0.7, 1.5)[i % 3], rpi=(24, 48)[i % 2], **base))
    for i, kt in enumerate(kts):
        out.append(C("%s k-tiles %d" % (tag, kt), M=m_base + bm + 1, Nout=nouts[(i + 1) % len(nouts)], Cin=bk * kt, res=(F32, F16, None)[i % 3],
                     out=(F16, F32)[i % 2], scale=(0.7, 1.0)[i % 2], rpi=(48, 24)[i % 2], **base))
    return out


def conv_edges(tag, bk, policy=None, wide=None, scalar=False, nouts=None, big=None):
    """IG_CONV2D: 3x3 with Cin in {32, 96, 160} (BK = 32) or 64 (BK = 64) so that tap and k-tile boundaries coincide and interleave;
    odd 7 x 9 maps, stride 2 on odd input, up = 2, tap_origin = 1, res_up = 2, and a 1x1"""
    cins = (32, 96, 160) if bk == 32 else (64, 64, 128)
    nn, n1 = nouts or ((72, 88) if scalar == "n" else (80, 64))
    pad = 12 if scalar == "ld" else 16
    b = dict(mode=CONV, policy=policy, wide=wide, pad=pad)
    b.update(big or {})
    n = b.pop("n", 3)
    return [
        C(tag + " 7x9", n=n, H=7, W=9, Cin=cins[0], Nout=nn, res=F16, **b),
        C(tag + " 7x9 stride2", n=n, H=7, W=9, stride=2, Cin=cins[1], Nout=n1, res=F32, out=F32, scale=0.7, **b),
        C(tag + " 5x7 up2 res_up2", n=n, H=5, W=7, up=2, Cin=cins[2], Nout=nn, res=F32, res_up=2, **b),
        C(tag + " 9x7 tap_origin stride2", n=n, H=9, W=7, stride=2, tap_origin=1, Cin=cins[1], Nout=nn, **b),
        C(tag + " 1x1 7x9", n=n, H=7, W=9, taps=1, Cin=cins[2], Nout=nn, res=F16, out=BF16, **b),
    ]


def temporal_edges(tag, bk, policy=None, wide=None, scalar=False, nouts=None, hw=20):
    cins = (32, 96, 160) if bk == 32 else (64, 64, 128)
    nn, n1 = nouts or ((72, 88) if scalar == "n" else (80, 64))
    pad = 12 if scalar == "ld" else 16
    b = dict(mode=TEMP, policy=policy, wide=wide, pad=pad)
    return [
        C(tag + " F1", b=3, F=1, HW=hw, Cin=cins[0], Nout=nn, res=F16, **b),
        C(tag + " F2", b=2, F=2, HW=hw + 3, Cin=cins[1], Nout=n1, res=F32, out=F32, scale=0.7, **b),
        C(tag + " F5", b=2, F=5, HW=hw, Cin=cins[2], Nout=nn, **b),
        C(tag + " F1 t_pad", b=3, F=1, HW=hw, Cin=cins[0], Nout=nn, t_pad=1, **b),
        C(tag + " F2 t_pad", b=2, F=2, HW=hw + 3, Cin=cins[1], Nout=nn, t_pad=1, res=F16, **b),
        C(tag + " F5 t_pad", b=2, F=5, HW=hw, Cin=cins[2], Nout=nn, t_pad=1, res=F32, **b),
    ]


FORCE = lambda t: {"CTRL_IGEMM_FORCE": t}          # noqa: E731
SMALL0 = {"CTRL_SMALL_TILES": "0"}
INL0, INLALL = {"CTRL_SPLITK_INLAUNCH": "0"}, {"CTRL_SPLITK_INLAUNCH": "all"}

# ------------------------------------------------------------------------------------------------------------------------------------
# THE TABLE: (kernel symbol, how the suite reaches it, cases)
# ------------------------------------------------------------------------------------------------------------------------------------
FORMS = []


def form(sym, how, cases):
    FORMS.append((sym, how, cases))


# ---- the !bk64 branch (Cin % 64 != 0): 64 x 64 x 32 by default, 128 x 128 x 32 from 192 tiles on; both epilogues; all modes ----
for md, mname in ((ROWS, "rows"), (CONV, "conv"), (TEMP, "temporal")):
    for swap, sc in ((True, False), (False, "n"), (False, "ld")):
        how = "Cin %% 64 != 0, < 192 tiles of 128^2%s" % ("" if swap else (", Nout %% 16 != 0" if sc == "n" else ", ld %% 8 != 0"))
        tag = "64x64x32 %s%s" % (mname, "" if swap else " scalar-" + sc)
        if md == ROWS:
            cs = rows_edges(tag, 64, 64, 32, 3, scalar=sc, ktiles=[1, 3, 5, 11], k_m=5)        # odd k-tile counts only: Cin % 64 != 0 is what selects the form
            cs += [C(tag + " k-tiles 1 M1", mode=ROWS, M=1, Nout=80 if sc != "n" else 72, Cin=32, pad=12 if sc == "ld" else 16)]
        elif md == CONV:
            cs = conv_edges(tag, 32, scalar=sc)
        else:
            cs = temporal_edges(tag, 32, scalar=sc)
        form(ring(64, 64, 32, 2, 2, 3, md, swap), how, cs)
    # 128 x 128 x 32 through the default choice: 192 tiles of 128^2 = 48 x 4 (Nout 512), M edges around the 48th tile
    for swap, sc in ((True, False), (False, "n"), (False, "ld")):
        tag = "128x128x32 %s%s" % (mname, "" if swap else " scalar-" + sc)
        nn = 4 * 128 + (8 if sc == "n" else 0)                                   # 5 tile columns when ragged
        pad = 12 if sc == "ld" else 16
        if md == ROWS:
            cs = [C("%s M%d" % (tag, m), mode=ROWS, M=m, Nout=nn, Cin=96, pad=pad, res=F32, out=F32, scale=0.7) for m in (48 * 128 - 127, 48 * 128, 48 * 128 + 1)]
        elif md == CONV:
            cs = [C(tag + " 47x43", mode=CONV, n=3, H=47, W=43, Cin=96, Nout=nn, pad=pad, res=F16),
                  C(tag + " 95x87 stride2", mode=CONV, n=3, H=95, W=87, stride=2, Cin=32, Nout=nn, pad=pad)]
        else:
            cs = [C(tag + " F3", mode=TEMP, b=2, F=3, HW=1031, Cin=96, Nout=nn, pad=pad, res=F16),
                  C(tag + " F3 t_pad", mode=TEMP, b=2, F=3, HW=1031, Cin=32, Nout=nn, pad=pad, t_pad=1)]
        form(ring(128, 128, 32, 2, 2, 3, md, swap), "Cin %% 64 != 0, >= 192 tiles of 128^2", cs)

# ---- Cin % 64 == 0, the fall-through chain: 128 x 128 x 64 (>= 192 tiles, eff > 0.8), 128 x 64 x 64 (>= 192 tiles of 128 x 64), 64 x 64 x 64 ----
for md, mname in ((ROWS, "rows"), (CONV, "conv"), (TEMP, "temporal")):
    pol = SMALL0 if md == ROWS else None         # rows: the small-tile policy would take the vector forms first
    for swap, sc in ((True, False), (False, "n"), (False, "ld")):
        sfx = "" if swap else " scalar-" + sc
        pad = 12 if sc == "ld" else 16
        # 64 x 64 x 64
        tag = "64x64x64 %s%s" % (mname, sfx)
        if md == ROWS:
            cs = rows_edges(tag, 64, 64, 64, 3, scalar=sc, policy=SMALL0)
        elif md == CONV:
            cs = conv_edges(tag, 64, scalar=sc)
        else:
            cs = temporal_edges(tag, 64, scalar=sc)
        form(ring(64, 64, 64, 2, 2, 3, md, swap), "Cin %% 64 == 0, few tiles%s" % (", CTRL_SMALL_TILES=0" if md == ROWS else ""), cs)
        # 128 x 64 x 64: Nout 192 (eff(128) = 0.75), 64 x 3 tiles of 128 x 64
        tag = "128x64x64 %s%s" % (mname, sfx)
        nn = 192 + (8 if sc == "n" else 0)
        if md == ROWS:
            cs = [C("%s M%d" % (tag, m), mode=ROWS, M=m, Nout=nn, Cin=64 * kt, pad=pad, policy=SMALL0, res=F16, scale=0.7)
                  for m, kt in ((64 * 128 - 127, 1), (64 * 128, 2), (64 * 128 + 1, 3), (64 * 128 - 1, 4), (64 * 128 + 37, 7))]
        elif md == CONV:
            cs = [C(tag + " 57x49", mode=CONV, n=3, H=57, W=49, Cin=64, Nout=nn, pad=pad, res=F32)]
        else:
            cs = [C(tag + " F3", mode=TEMP, b=2, F=3, HW=1399, Cin=64, Nout=nn, pad=pad)]
        form(ring(128, 64, 64, 2, 2, 3, md, swap), "Cin %% 64 == 0, >= 192 tiles of 128 x 64, eff(128) <= 0.8", cs)
        # 128 x 128 x 64 (8 waves, 4 stages): 48 x 4 tiles
        tag = "128x128x64 %s%s" % (mname, sfx)
        nn = 512 + (8 if sc == "n" else 0)
        if md == ROWS:
            cs = [C("%s M%d" % (tag, m), mode=ROWS, M=m, Nout=nn, Cin=64 * kt, pad=pad, policy=SMALL0, res=F32, out=F32)
                  for m, kt in ((48 * 128 - 127, 1), (48 * 128, 2), (48 * 128 + 1, 3), (48 * 128 + 1, 4), (48 * 128 + 37, 5), (48 * 128 - 1, 9))]
        elif md == CONV:
            cs = [C(tag + " 47x43", mode=CONV, n=3, H=47, W=43, Cin=64, Nout=nn, pad=pad, res=F16)]
        else:
            cs = [C(tag + " F3", mode=TEMP, b=2, F=3, HW=1031, Cin=64, Nout=nn, pad=pad, t_pad=1)]
        form(ring(128, 128, 64, 2, 4, 4, md, swap), "Cin %% 64 == 0, >= 192 tiles of 128^2%s" % (", CTRL_SMALL_TILES=0" if md == ROWS else ""), cs)

# ---- the paired split-operand walk (a_split = 2) at Cin / 2 = 64: two k-tiles (64-deep) / four (32-deep) per tap ----
form(ring(64, 64, 64, 2, 2, 3, CONV), "a_split = 2, Cin / 2 = 64, few tiles",
     [C("paired 64x64x64 conv 7x9", mode=CONV, n=3, H=7, W=9, Cin=128, Nout=80, a_split=2, res=F32),
      C("paired 64x64x64 conv 1x1", mode=CONV, n=3, H=7, W=9, taps=1, Cin=128, Nout=64, a_split=2)])
form(ring(64, 64, 64, 2, 2, 3, ROWS), "a_split = 2, Cin / 2 = 64, rows", [C("paired 64x64x64 rows", mode=ROWS, M=65, Nout=80, Cin=128, a_split=2, res=F16)])
form(wide8(4, CONV), "a_split = 2, Cin / 2 = 64, set_igemm_wide(2)", [C("paired wide4 conv 7x9", mode=CONV, n=5, H=7, W=9, Cin=128, Nout=256, a_split=2, wide=2, res=F32)])
form(wide8(5, CONV), "a_split = 2, Cin / 2 = 64, set_igemm_wide(2)", [C("paired wide5 conv 9x7 stride2", mode=CONV, n=5, H=9, W=7, stride=2, Cin=128, Nout=320, a_split=2, wide=2)])

# ---- the small-tile policy (rows, vector epilogue): 64 x 64 x 64 below 512 tiles, 128 x 128 x 32 from 512 tiles on ----
form(ring(64, 64, 64, 2, 2, 3, ROWS), "default small-tile policy: rows, < 512 tiles, Nout <= 1280",
     [C("small-tiles 64x64x64 M130", mode=ROWS, M=130, Nout=80, Cin=192, res=F16), C("small-tiles 64x64x64 M65 K64", mode=ROWS, M=65, Nout=64, Cin=64, res=F32, out=F32)])
form(ring(128, 128, 32, 2, 2, 3, ROWS), "default small-tile policy: rows, >= 512 tiles of 128^2",
     [C("small-tiles 128x128x32 M%d" % m, mode=ROWS, M=m, Nout=512, Cin=64 * kt, res=F16, scale=0.7) for m, kt in ((128 * 128 - 127, 1), (128 * 128 + 1, 2))])

# ---- the pinned form of the encoder plans ----
form(ring(64, 64, 64, 2, 2, 3, ROWS), "ops.igemm(pinned=True) -> op_igemm_pinned", rows_edges("pinned", 64, 64, 64, 3, pinned=True) +
     [C("pinned M4100 (the dispatcher would take a bigger tile)", mode=ROWS, M=4100, Nout=1024, Cin=128, pinned=True, res=F16)])

# ---- forced tiles (CTRL_IGEMM_FORCE; rows, vector epilogue) ----
for name, (bm, bn, bk, wm, wn, ns) in (("128x128x32", (128, 128, 32, 2, 2, 3)), ("128x64x64", (128, 64, 64, 2, 2, 3)), ("64x64x64", (64, 64, 64, 2, 2, 3)),
                                       ("128x128x64", (128, 128, 64, 2, 4, 4)), ("128x256", (128, 256, 32, 2, 4, 3)), ("256x128", (256, 128, 32, 4, 2, 3)),
                                       ("4w256x128", (256, 128, 32, 2, 2, 3)), ("4w128x256", (128, 256, 32, 1, 4, 3))):
    form(ring(bm, bn, bk, wm, wn, ns, ROWS), "CTRL_IGEMM_FORCE=" + name, rows_edges("force " + name, bm, bn, bk, ns, policy=FORCE(name)))

# ---- the 8-phase wide tiles: forced (set_igemm_wide(2) / CTRL_IGEMM_FORCE=wide), and once by default ----
for ni in (4, 5):
    bn = 64 * ni
    cs = rows_edges("wide%d" % ni, 256, bn, 64, 2, wide=2, ktiles=[1, 2, 3, 9, 11], nouts=[bn])          # (Nout % BN == 0 is a precondition of the form)
    cs += [C("wide%d M257 2 tile columns" % ni, mode=ROWS, M=257, Nout=2 * bn, Cin=192, wide=2, res=F32, out=F32, mirror=True, scale=0.7),
           C("wide%d split mirror" % ni, mode=ROWS, M=300, Nout=bn, Cin=128, wide=2, res=F32, out=F32, mirror="split"),
           C("wide%d transposed out" % ni, mode=ROWS, M=3 * 136, L=136, Nout=bn, Cin=128, wide=2, res=F16, out=F32, scale=0.7),
           C("wide%d scale2 range" % ni, mode=ROWS, M=255, Nout=bn, Cin=64, wide=2, scale=0.7, scale2=0.18, scale2_from=64, scale2_to=128)]
    form(wide8(ni, ROWS), "set_igemm_wide(2)", cs)
    form(wide8(ni, ROWS), "CTRL_IGEMM_FORCE=wide", [C("force wide%d" % ni, mode=ROWS, M=257, Nout=bn, Cin=192, policy=FORCE("wide"), res=F16)])
    form(wide8(ni, CONV), "set_igemm_wide(2)", conv_edges("wide%d conv" % ni, 64, wide=2, nouts=(bn, 2 * bn), big=dict(n=5)))
    form(wide8(ni, TEMP), "set_igemm_wide(2)", temporal_edges("wide%d temporal" % ni, 64, wide=2, nouts=(bn, 2 * bn), hw=52))
    mdef = (160 if ni == 5 else 200) * 256
    form(wide8(ni, ROWS), "default: the grid fills the chip", [C("wide%d default M%d" % (ni, mdef - 255), mode=ROWS, M=mdef - 255, Nout=bn, Cin=64, res=F16)])
    form(wide8(ni, CONV), "default: the grid fills the chip", [C("wide%d conv default" % ni, mode=CONV, n=4, H=113, W=113 if ni == 4 else 91, Cin=64, Nout=bn)])
    form(wide8(ni, TEMP), "default: the grid fills the chip", [C("wide%d temporal default" % ni, mode=TEMP, b=2, F=3, HW=8533 if ni == 4 else 6827, Cin=64, Nout=bn)])

# ---- the BK = 32 ring forms of the wide tiles (vector epilogue only): Cin % 64 != 0 (or set_igemm_wide(0)) on a filled grid ----
for md, mname in ((ROWS, "rows"), (CONV, "conv"), (TEMP, "temporal")):
    for bn, nout, ntm in ((256, 1280, 40), (320, 640, 80)):
        tag = "256x%dx32 %s" % (bn, mname)
        if md == ROWS:
            cs = [C("%s M%d k-tiles %d" % (tag, m, kt), mode=ROWS, M=m, Nout=nout, Cin=32 * kt, res=(F16, F32)[kt % 2], scale=0.7)
                  for m, kt in ((ntm * 256 - 255, 1), (ntm * 256, 3), (ntm * 256 + 1, 5), (ntm * 256 - 1, 7))]
            cs += [C("%s wide off, Cin 128" % tag, mode=ROWS, M=ntm * 256 - 100, Nout=nout, Cin=128, wide=0, policy=SMALL0, res=F16)]
        elif md == CONV:
            hh = {40: (59, 58), 80: (83, 83)}[ntm]
            cs = [C(tag + " %dx%d Cin96" % hh, mode=CONV, n=3, H=hh[0], W=hh[1], Cin=96, Nout=nout, res=F16),
                  C(tag + " %dx%d Cin32 stride2" % (2 * hh[0] - 1, 2 * hh[1] - 1), mode=CONV, n=3, H=2 * hh[0] - 1, W=2 * hh[1] - 1, stride=2, Cin=32, Nout=nout)]
        else:
            hw = (ntm * 256 - 100) // 6
            cs = [C(tag + " F3 Cin96", mode=TEMP, b=2, F=3, HW=hw, Cin=96, Nout=nout, res=F16),
                  C(tag + " F3 Cin32 t_pad", mode=TEMP, b=2, F=3, HW=hw, Cin=32, Nout=nout, t_pad=1)]
        form(ring(256, bn, 32, 2, 4, 4, md), "Cin %% 64 != 0 (or set_igemm_wide(0)), >= %d tiles of 256 x %d" % (200 if bn == 256 else 160, bn), cs)

# ---- the two-workgroup tiles of the M >= 65536 branches ----
form(ring(128, 256, 32, 2, 4, 3, ROWS), "M >= 65536, fp32 stream, Ktot <= 1024",
     [C("large-M f32 stream", mode=ROWS, M=65536 + 129, Nout=256, Cin=96, res=F32, out=F32, mirror=True)])
form(ring(128, 256, 32, 2, 4, 3, ROWS), "M >= 65536, fp16 residual, Ktot <= 512 (CTRL_SHORTK_PAIR)",
     [C("large-M fp16 stream", mode=ROWS, M=65536 + 1, Nout=256, Cin=64, res=F16)])

# ---- split-K: rows / conv; the finish kernel and the in-launch reduction; the smallest split, a one-k-tile last split, the paired walk ----
# igemm_splitk_factor: one 256-row tile -> 16 splits, capped by (Ktot / 32) / splits >= 16 and Ktot >= 2048.
#   * smallest: Ktot = 2048 -> 4 splits of 8 (64-deep) k-tiles;
#   * last split owns ONE k-tile: only 16 splits of the 64-deep kernel can (last = nk - 15 ceil(nk / 16) = 1 at nk = 241, Ktot 15424);
#     the 32-deep ring kernel never gets there (nk32 / sk >= 16 leaves its last split >= 17 - sk k-tiles, and 16 splits need nk32 >= 256,
#     where the last split owns 16), so it is run at its smallest last split instead: 65 k-tiles over 4 splits (17, 17, 17, 14);
#   * paired walk: split-K needs Ktot >= 2048, i.e. Cin >= 228 for a 3x3 problem, so Cin / 2 = 64 (Ktot 1152) cannot split; the split
#     case runs at Cin / 2 = 128 (a split never cuts a (hi, lo) pair: 36 k-tiles as 10, 10, 10, 6), and the Cin / 2 = 64 walk is run
#     unsplit on the wide and the ring kernels in FORMS above.
SPLITK = []
for ni, nout in ((4, 256), (5, 320)):
    SPLITK += [
        (wide8(ni, ROWS), C("splitk wide%d rows smallest K2048" % ni, mode=ROWS, M=130, Nout=nout, Cin=2048, sk=4, res=F32)),
        (wide8(ni, ROWS), C("splitk wide%d rows last split owns one k-tile K15424" % ni, mode=ROWS, M=257, Nout=nout, Cin=15424, sk=16, res=F16, scale=0.7)),
        (wide8(ni, CONV), C("splitk wide%d conv 7x9 Cin256" % ni, mode=CONV, n=3, H=7, W=9, Cin=256, Nout=nout, sk=4, res=F16)),
        (wide8(ni, CONV), C("splitk wide%d conv paired Cin/2=128" % ni, mode=CONV, n=2, H=8, W=8, Cin=256, Nout=nout, a_split=2, sk=4, res=F32)),
        (ring(256, 64 * ni, 32, 2, 4, 4, ROWS), C("splitk ring 256x%d rows K2080" % (64 * ni), mode=ROWS, M=130, Nout=nout, Cin=2080, sk=4, res=F16)),
        (ring(256, 64 * ni, 32, 2, 4, 4, CONV), C("splitk ring 256x%d conv Cin288" % (64 * ni), mode=CONV, n=2, H=8, W=8, Cin=288, Nout=nout, sk=5, res=F32)),
    ]



def splitk_variant(sym, c, reduce):
    """the SPLITK case `c` under one of the three reductions: "finish" | "inlaunch" | "inlaunch_tickets" """
    c = Case(c)
    ringk = sym.startswith("igemm_kernel")
    # the ring kernels have no in-launch reduction: the finish kernel follows whatever the policy says
    c.update(splitk="finish" if (reduce == "finish" or ringk) else "inlaunch", tickets=(reduce == "inlaunch_tickets" and not ringk),
             policy=INL0 if reduce == "finish" else INLALL)
    return c


ALL = [(sym, how, c) for sym, how, cs in FORMS for c in cs]
