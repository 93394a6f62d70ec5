"""Host self-test of the fused feed-forward's forms suite (tests/ffn_forms.py, tests/test_gpu_ffn_forms.py): the case table is complete, the
derived bound holds for an fp32 emulation of the kernel's arithmetic and rejects planted errors, the W2 pack restated on the host is a
bijection, and ctrl_op_ffn / ctrl_op_ffn_group refuse what the kernel cannot run before anything is launched.  No GPU."""
import ctypes as C
import itertools

import pytest
import torch

import helpers  # noqa: F401  (puts the repository root on the path)
import ffn_forms as F


def _ratio(case_id, planted=None):
    """worst |emulation - ref| / bound over the case's outputs (master and mirror)"""
    c = F.CASE_BY_ID[case_id]
    f = F.FORMS[c["form"]]
    ref, b32, b16 = F.reference(case_id)
    out, mir = F.emulate(case_id, planted)
    r = F.check(out, ref, b32 if f["out"] == torch.float32 else b16)
    return max(r, F.check(mir, ref, b16)) if mir is not None else r


def test_tables_are_complete():
    """kinds x M, kinds x epilogue forms, M classes x epilogue forms, and every stride variant with a form it acts on, per kind"""
    ids = [c["id"] for c in F.CASES]
    assert len(set(ids)) == len(ids)
    have = lambda *keys: {tuple(c[k] if k != "mclass" else F.m_class(c["M"]) for k in keys) for c in F.CASES}      # noqa: E731
    assert have("kind", "M") == set(itertools.product(F.KINDS, F.MS))
    assert have("kind", "form") == set(itertools.product(F.KINDS, F.FORMS))
    assert have("mclass", "form") == set(itertools.product({F.m_class(M) for M in F.MS}, F.FORMS))
    assert {F.m_class(M) for M in F.MS} == {"below a tile", "one full tile", "ragged tiles", "ten tiles"}
    assert have("kind", "stride") == set(itertools.product(F.KINDS, F.STRIDES))
    for c in F.CASES:
        assert F.stride_matters(c["form"], c["stride"]), c["id"]
    for s in F.STRIDES.values():
        assert all(v % 8 == 0 and v >= 512 for v in s)
    # last row tiles of 1, 16, 127 and 128 rows; groups need four members at one tile and at ten
    assert {(M - 1) % 128 + 1 for M in F.MS} == {1, 16, 127, 128}
    for M in (127, 1153):
        assert len({(c["form"], c["stride"]) for c in F.CASES if c["M"] == M}) >= 4, M


def test_every_hidden_unit_reaches_an_output_in_the_constructed_cases():
    """sparse / gate: W2 has few non-zeros, so a unit the kernel mis-places shows only if SOME output reads it -- every unit of every
    chunk does, the four units of an output channel lie in four chunks and four k-steps, and W1's non-zeros cover all eight k-tiles"""
    for kind in ("sparse", "gate"):
        reached = torch.zeros(F.H, dtype=torch.bool)
        for c in F.CASES:
            if c["kind"] != kind:
                continue
            p = F.problem(c["id"])
            reached |= (p["w2"] != 0).any(0)
            tiles = (p["w1"] != 0).view(2 * F.H, 8, 64).any(2)
            assert bool(tiles.any(0).all()), c["id"]
            if kind == "sparse":
                assert int((p["w2"] != 0).sum(1).min()) == 4 and int((p["w1"] != 0).sum(1).max()) <= 3
        if kind == "sparse":
            assert bool(reached.all()), "%s: %d hidden units reach no output" % (kind, int((~reached).sum()))
    union = torch.zeros(F.H, dtype=torch.bool)
    for c in F.CASES:
        if c["kind"] in ("sparse", "gate"):
            union |= (F.problem(c["id"])["w2"] != 0).any(0)
    assert bool(union.all())
    units = [F.sparse_w2_units(n) for n in range(F.D)]
    assert sorted(u for us in units for u in us) == list(range(F.H))
    for us in units:
        assert len({u // F.HC for u in us}) == 4 and {F.unit_kstep(u) for u in us} == {0, 1, 2, 3}
    assert {u // F.HC for us in units for u in us} == set(range(F.NCH))


def test_gelu_error_term_is_derived_and_above_the_emulation():
    """the constants of the derivation (tests/ffn_forms.py) evaluated from gelu_erf_f's coefficients, and the fp32 emulation (exact rcp
    and exp2) against the exact GELU on a 2M-point grid over [-12, 12]: its worst error over |x| is the floor the derived term must
    clear, and its worst err / eg is recorded"""
    t = torch.linspace(1e-6, 1.0, 200001, dtype=torch.float64)
    c = [a / 2 for a in F.GELU_A]
    z = (1.0 / t - 1.0) / F.GELU_P
    e = torch.exp(-z * z)
    sens = (sum((k + 1) * ck * t ** (k + 1) for k, ck in enumerate(c)).abs() * e).max().item()
    assert sens <= F.GELU_SENS_T, sens
    q5 = c[4] * t; s4 = c[3] + q5; q4 = t * s4; s3 = c[2] + q4; q3 = t * s3; s2 = c[1] + q3; q2 = t * s2; s1 = c[0] + q2; hp = t * s1      # noqa: E702
    horner = sum(v.abs().max().item() for v in (q5, s4, q4, s3, q3, s2, q2, s1, hp))
    assert horner <= F.GELU_SUM_HORNER, horner
    assert (hp * e).max().item() <= 0.5 + 1e-7          # P(t) e^(-z^2) / 2 = erfc(z) / 2 (+ the fit's own error)
    a = torch.linspace(0.0, 40.0, 400001, dtype=torch.float64)
    assert (a * torch.exp2(-a) * 0.6931471805599453).max().item() <= 0.37
    x = torch.linspace(-12.0, 12.0, 2000001, dtype=torch.float64).float()
    x = x[x != 0]
    err = (F.gelu_erf_f_emul(x).double() - F.gelu64(x.double())).abs()
    floor = (err / x.double().abs()).max().item()
    ratio = (err / F.gelu_err(x.double().abs(), F.gelu64(x.double()).abs())).max().item()
    print("GELU-CHECK derived C_G %.3e |g| (%s); emulation floor %.3e |g|; worst err / eg %.3f" % (
        F.GELU_C, ", ".join("%s %.2e" % kv for kv in F.GELU_TERMS), floor, ratio))
    assert 2.0e-7 < floor < F.GELU_C and ratio < 1.0, (floor, ratio)
    # the approximations a wrong kernel might use are far outside eg
    for act in ("tanh", "quick"):
        bad = ((F.gelu_erf_f_emul(x, act).double() - F.gelu64(x.double())).abs() / F.gelu_err(x.double().abs(), F.gelu64(x.double()).abs())).max().item()
        assert bad > 50, (act, bad)


def test_emulation_stays_inside_the_bound_on_every_case():
    worst = {}
    for c in F.CASES:
        r = _ratio(c["id"])
        assert r <= 1.0, "%s: the fp32 emulation is %.3f of the bound" % (c["id"], r)
        worst[c["kind"]] = max(worst.get(c["kind"], 0.0), r)
    print("FFN-CHECK emulation, worst err/bound per kind: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    # the bound is not loose where it matters: rounding P to fp16 ties takes the constructed kinds close to it
    assert worst["gate"] > 0.5 and worst["sparse"] > 0.5


def _applies(c, planted):
    if planted == "last_tile_rows_shifted":
        return (c["M"] - 1) % 128 + 1 >= 2          # a one-row tile has nothing to shift
    if c["kind"] == "dense":
        return c["M"] >= 127                          # one unit is 1 of 2048 addends: a dense case needs a tile's worth of rows to see it
    return True


@pytest.mark.parametrize("planted", F.PLANTED)
def test_bound_rejects_planted_errors(planted):
    """which kind catches what (ffn_forms.MUST_REJECT): the W2 layout errors, the exchanged halves and the shifted rows show in every kind;
    a bias from the neighbouring chunk cannot show in `gate` (its b1 is the same in every chunk); only `gate` tells tanh from erf; and a
    P that was NOT rounded to fp16 must pass everywhere -- the bound allows for that rounding, it does not demand it"""
    must = F.MUST_REJECT[planted]
    seen = {k: [] for k in F.KINDS}
    for c in F.CASES:
        if not _applies(c, planted):
            continue
        r = _ratio(c["id"], planted)
        seen[c["kind"]].append(r)
        if c["kind"] in must:
            assert r > 1.0, "%s: planted %s passes (%.3f of the bound)" % (c["id"], planted, r)
        elif planted == "p_not_fp16" or (planted, c["kind"]) == ("b1_of_next_chunk", "gate"):
            assert r <= 1.0, "%s: %s must pass (%.3f of the bound)" % (c["id"], planted, r)
    print("FFN-CHECK planted %-26s err/bound min..max per kind: %s" % (planted, ", ".join(
        "%s %.3g..%.3g" % (k, min(v), max(v)) for k, v in seen.items() if v)))
    for k in must:
        assert seen[k], (planted, k)
    if planted == "tanh_gelu":          # a dense random case cannot tell the activations apart: the gap `gate` closes
        assert max(seen["dense"]) <= 1.0 and min(seen["gate"]) > 50


def test_w2_pack_restated_on_the_host_is_a_bijection():
    idx = F.w2_pack_index()
    assert idx.numel() == F.D * F.H and torch.equal(torch.sort(idx).values, torch.arange(F.D * F.H))
    # k-step kap of chunk c holds, per output channel, the 32 units whose bits (4, 1) are kap: what FF_GEGLU stores for that k-step
    n, u = idx // F.H, idx % F.H
    pack = torch.stack([n, u], 1).view(4, F.D, 512, 2)
    assert torch.equal(pack[..., 0], torch.arange(F.D).view(1, F.D, 1).expand(4, F.D, 512))
    col = torch.arange(512)
    assert torch.equal(pack[..., 1] // F.HC, (torch.arange(4).view(4, 1, 1) * 4 + (col >> 7).view(1, 1, 512)).expand(4, F.D, 512))
    kap = ((col & 127) >> 5).view(1, 1, 512).expand(4, F.D, 512)
    uu = pack[..., 1] % F.HC
    assert torch.equal(2 * ((uu >> 4) & 1) + ((uu >> 1) & 1), kap)
    rows = F.geglu_pack_rows()
    assert torch.equal(torch.sort(rows).values, torch.arange(2 * F.H))
    # chunk c of the W1 pack = rows 256 c .. 256 c + 255 = hidden units 128 c .. 128 c + 127 and their gates
    for c in (0, 7, 15):
        blk = rows[256 * c:256 * c + 256]
        assert set(blk.tolist()) == set(range(128 * c, 128 * c + 128)) | set(range(F.H + 128 * c, F.H + 128 * c + 128))


# ---------------------------------------------------------------------------------------------------------------------------
# Refusals (CPU: ffn_check runs before the first HIP call, so a refusal is the check's own message, never a launch error)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib as L, ops
    M = 16
    t = dict(x=torch.zeros(M, 512, dtype=torch.float16), w1=torch.zeros(4096, 512, dtype=torch.float16), b1=torch.zeros(4096),
             w2=torch.zeros(512, 2048, dtype=torch.float16), out=torch.zeros(M, 512), mir=torch.zeros(M, 512, dtype=torch.float16),
             res=torch.zeros(M, 512), b2=torch.zeros(512), bx=torch.zeros(M, 512), mix=torch.zeros(1))

    def make(**kw):
        return ops.ffn_desc(t["x"], t["w1"], t["b1"], t["w2"], t["out"], b2=t["b2"], res=t["res"], out16=t["mir"], **kw)
    return L, ops, t, make


def _refused(L, descs, n, needle):
    arr = (L.FfnDesc * max(len(descs), 1))(*descs)
    lib = L.lib()
    rc = lib.ctrl_op_ffn_group(arr, n, None)
    msg = (lib.ctrl_last_error() or b"").decode()
    assert rc != 0 and "ffn" in msg and needle in msg, (rc, msg, needle)
    if n == 1:
        assert lib.ctrl_op_ffn(C.byref(arr[0]), None) != 0
        assert needle in (lib.ctrl_last_error() or b"").decode()


def test_ffn_entry_points_refuse_before_any_launch(good):
    L, ops, t, make = good
    for n in (0, 5):
        _refused(L, [make()] * 5, n, "group size")
    _refused(L, [make(), make(M=8)], 2, "same M")

    def one(needle, edit, **kw):
        d = make(**kw)
        edit(d)
        _refused(L, [d], 1, needle)

    def setf(**fields):
        def edit(d):
            for k, v in fields.items():
                obj, name = (d, k) if hasattr(d, k) else (d.out.seg[0], k[4:]) if k.startswith("seg_") else (d.out, k)
                setattr(obj, name, v)
        return edit

    one("16-byte aligned", setf(ldx=520))
    one("[M][512]", setf(Nout=256))
    one("[M][512]", setf(M=0))
    one("null operand", setf(W2p=None))
    for name in ("X", "W1", "b1", "W2p"):
        one("16-byte aligned", lambda d, name=name: setattr(d, name, getattr(d, name) + 8))
    # what the swapped epilogue asks for (section E)
    one("multiples of 8", setf(seg_ld=516))
    one("multiples of 8", setf(seg_ld=504))
    one("multiples of 8", setf(ldres=516))
    one("multiples of 8", setf(ld16=516))
    one("multiples of 8", setf(ld_blend=516), blend_mix=t["mix"], blend_x=t["bx"])
    one("16-byte aligned", lambda d: setattr(d.out.seg[0], "out", d.out.seg[0].out + 8))
    one("16-byte aligned", lambda d: setattr(d.out, "res", d.out.res + 8))
    one("16-byte aligned", lambda d: setattr(d.out, "out16", d.out.out16 + 8))
    one("16-byte aligned", lambda d: setattr(d.out, "bias", d.out.bias + 4))
    one("16-byte aligned", lambda d: setattr(d.out, "blend_x", d.out.blend_x + 8), blend_mix=t["mix"], blend_x=t["bx"])
    # descriptor fields the epilogue would act on and this op does not offer
    one("no output scale", setf(scale=0.5))
    one("no output scale", setf(out16_lo_off=512))
    one("no output scale", setf(blend_x=None), blend_mix=t["mix"], blend_x=t["bx"])
    one("fp16 or fp32 rows", setf(seg_dtype=L.BF16))
    one("fp16 or fp32 rows", setf(seg_out=None))
    one("one row-major output segment", setf(nseg=2))
    one("one row-major output segment", setf(seg_fmt=ops.SEG_TRANSPOSED))
    one("one row-major output segment", setf(seg_col_begin=16))
    one("one row-major output segment", setf(seg_ncols=256))
    one("one row-major output segment", setf(geglu=1))
    one("one row-major output segment", setf(act=1))
    one("one row-major output segment", setf(rowvec=t["b2"].data_ptr()))
    one("one row-major output segment", setf(res_up=2))
    one("one row-major output segment", setf(scale2_from=8))
    one("beyond 2^32", setf(seg_ld=2 ** 31))
