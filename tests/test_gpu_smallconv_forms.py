"""The small 3x3 convolutions (csrc/smallconv.hip) at their edges: every template form of the direct kernel -- the two fp32 stems that write
the backbone UNets' residual stream among them -- and of the MFMA kernel against an fp64 conv2d (+ SiLU) and the bound of
tests/smallconv_forms.py, element by element, inputs inside NaN guards and outputs inside poisoned ones.  The first section needs no GPU:
the tables are complete and the ops refuse what the kernels cannot run."""
import itertools

import pytest
import torch

import helpers
import smallconv_forms as S


# ---------------------------------------------------------------------------------------------------------------------------
# host section
# ---------------------------------------------------------------------------------------------------------------------------
def test_tables_are_complete():
    ids = [c["id"] for c in S.DIRECT_CASES + S.MFMA_CASES]
    assert len(set(ids)) == len(ids)
    have = lambda cases, *keys: {tuple(c[k] for k in keys) for c in cases}      # noqa: E731
    # the five template forms of the direct kernel: NCHW in (Cin 3 and 4 from f32, f16 and bf16), channels-last fp16 in (Cin 16 and 32), the
    # fp32 stems from NCHW (Cin 4 and 8) and from fp32 rows (Cin 8); each with one block of 16 channels, three of 16 and two of 32
    assert have(S.DIRECT_CASES, "op", "Cin", "layout", "dtype") >= {
        ("direct", 3, "nchw", torch.float32), ("direct", 3, "nchw", torch.float16), ("direct", 3, "nchw", torch.bfloat16),
        ("direct", 4, "nchw", torch.float32), ("direct", 4, "nchw", torch.float16), ("direct", 4, "nchw", torch.bfloat16),
        ("direct", 16, "nhwc", torch.float16), ("direct", 32, "nhwc", torch.float16),
        ("stem", 4, "nchw", torch.float32), ("stem", 8, "nchw", torch.float32), ("rows", 8, "nhwc", torch.float32)}
    assert have(S.DIRECT_CASES, "form", "Cout") == set(itertools.product(S.DIRECT_FORMS, S.COUTS))
    for form, (op, _, _, _) in S.DIRECT_FORMS.items():
        cs = [c for c in S.DIRECT_CASES if c["form"] == form]
        npix = {c["N"] * S.out_hw(c)[0] * S.out_hw(c)[1] for c in cs}
        assert {255, 256, 257} <= npix and any(c["N"] == 5 and (c["H"], c["W"]) == (9, 7) for c in cs), form
        assert {c["bias"] for c in cs} == {False, True}, form
        if op == "direct":
            assert {c["silu"] for c in cs} == {False, True}, form
            s2 = [(c["H"] % 2, c["W"] % 2) for c in cs if c["stride"] == 2]
            assert (1, 1) in s2 and (0, 0) in s2, form
        else:
            assert all(c["stride"] == 1 and not c["silu"] for c in cs), form
    assert have(S.MFMA_CASES, "Cin", "Cout") == {(16, 16), (16, 32), (32, 16), (32, 32)}
    for form in {c["form"] for c in S.MFMA_CASES}:
        cs = [c for c in S.MFMA_CASES if c["form"] == form]
        assert {S.out_hw(c)[1] for c in cs} == {15, 16, 17, 33} and {S.out_hw(c)[0] for c in cs} == {7, 8, 9, 17}, form
        assert {c["bias"] for c in cs} == {False, True} and all(c["N"] == 2 and not c["silu"] for c in cs), form
        s2 = [(c["H"] % 2, c["W"] % 2) for c in cs if c["stride"] == 2]
        assert (1, 1) in s2 and (0, 0) in s2, form


def test_bound_rejects_a_planted_error_and_accepts_the_fp32_result():
    """the checker itself: an fp32 conv2d of torch's stays inside the bound of every case; one tap of one channel dropped, or the result
    shifted by one pixel, does not"""
    import torch.nn.functional as Fn
    for c in S.DIRECT_CASES[::5] + S.MFMA_CASES[::5]:
        x, w, b = S.problem(c["id"])
        ref, bound = S.reference(c["id"])
        odt = torch.float32 if c["op"] in ("stem", "rows") else torch.float16

        def run(wt):
            y = Fn.conv2d(x.float(), wt, b, stride=c["stride"], padding=1)
            return (Fn.silu(y) if c["silu"] else y).permute(0, 2, 3, 1).to(odt).double()
        assert float(((run(w) - ref).abs() / bound).max()) <= 1.0, c["id"]
        w_bad = w.clone()
        w_bad[0, 0, 1, 1] = 0.0          # the centre tap of channel 0 -> 0: present at every pixel
        assert float(((run(w_bad) - ref).abs() / bound).max()) > 1.0, c["id"]
        assert float(((torch.roll(run(w), 1, 2) - ref).abs() / bound).max()) > 1.0, c["id"]


def test_small_conv_ops_refuse_what_the_kernels_cannot_run():
    """before any launch (no GPU here): an unsupported Cin, Cout % 16 != 0, a stride other than 1 | 2, and misaligned pointers for every
    form that moves 16-byte pieces"""
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib as L
    lib = L.lib()
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    assert p % 16 == 0

    def refused(rc, needle):
        msg = (lib.ctrl_last_error() or b"").decode()
        assert rc != 0 and needle in msg, (rc, msg, needle)

    # direct: (in, in_dtype, in_nchw, w, bias, out, N, Cin, Cout, Hin, Win, stride, silu, stream)
    d = lambda **k: lib.ctrl_op_conv3x3_direct(*[L.C.c_void_p(v) if i in (0, 3, 4, 5, 13) else v for i, v in enumerate([      # noqa: E731
        k.get("inp", p), L.F16, k.get("nchw", 0), p, None, k.get("out", p), 1, k.get("Cin", 16), k.get("Cout", 16), 8, 8, k.get("stride", 1), 0, None])])
    refused(d(Cin=5), "unsupported")
    refused(d(Cin=16, nchw=1), "unsupported")
    refused(d(Cin=3, nchw=0), "unsupported")
    refused(d(Cout=24), "multiple of 16")
    refused(d(stride=3), "stride")
    refused(d(out=p + 8), "16-byte aligned")
    refused(d(inp=p + 8), "16-byte aligned")
    # small_mfma: (x, w, bias, out, N, Cin, Cout, Hin, Win, stride, silu, stream)
    m = lambda **k: lib.ctrl_op_conv3x3_small_mfma(L.C.c_void_p(k.get("x", p)), L.C.c_void_p(k.get("w", p)), L.C.c_void_p(k.get("bias", p)),      # noqa: E731
                                                   L.C.c_void_p(k.get("out", p)), 1, k.get("Cin", 16), k.get("Cout", 16), 8, 8, k.get("stride", 1), 0, None)
    refused(m(Cin=8), "16 or 32")
    refused(m(Cout=48), "16 or 32")
    refused(m(stride=4), "stride")
    for name in ("x", "w", "out"):
        refused(m(**{name: p + 8}), "16-byte aligned")
    refused(m(bias=p + 4), "16-byte aligned")
    # the stems: (in, in_dtype, w, bias, out, N, Cin, Cout, H, W, stream) / (in, w, bias, out, N, Cin, Cout, H, W, stream)
    vp = L.C.c_void_p
    refused(lib.ctrl_op_conv3x3_direct_f32(vp(p), L.F32, vp(p), None, vp(p), 1, 3, 16, 8, 8, None), "Cin must be 8")
    refused(lib.ctrl_op_conv3x3_direct_f32(vp(p), L.F32, vp(p), None, vp(p), 1, 4, 24, 8, 8, None), "multiple of 16")
    refused(lib.ctrl_op_conv3x3_direct_f32(vp(p), L.F32, vp(p), None, vp(p + 8), 1, 4, 16, 8, 8, None), "16-byte aligned")
    refused(lib.ctrl_op_conv3x3_direct_f32(None, L.F32, vp(p), None, vp(p), 1, 4, 16, 8, 8, None), "bad arguments")
    refused(lib.ctrl_op_conv3x3_rows_f32(vp(p), vp(p), None, vp(p), 1, 4, 16, 8, 8, None), "Cin must be 8")
    refused(lib.ctrl_op_conv3x3_rows_f32(vp(p), vp(p), None, vp(p), 1, 8, 40, 8, 8, None), "multiple of 16")
    refused(lib.ctrl_op_conv3x3_rows_f32(vp(p + 8), vp(p), None, vp(p), 1, 8, 16, 8, 8, None), "16-byte aligned")
    refused(lib.ctrl_op_conv3x3_rows_f32(vp(p), vp(p), None, vp(p + 8), 1, 8, 16, 8, 8, None), "16-byte aligned")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU section
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _assert_close(out, ref, bound, what):
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite outputs (a guard reached a kept element)" % (what, int((~torch.isfinite(o)).sum()))
    err = (o - ref).abs()
    worst = float((err / bound).max())
    rel = float(err.max() / ref.abs().max().clamp_min(1e-12))
    print("CONV-CHECK %-44s worst err/bound %.3f  rel_inf %.2e" % (what, worst, rel))
    bad = err > bound
    if bool(bad.any()):
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond the fp32-accumulation bound (worst err/bound %.2f); first at (n, y, x, c) = %s: got %.6g "
                             "want %.6g bound %.3g" % (what, int(bad.sum()), bad.numel(), worst, first, float(o[first]), float(ref[first]),
                                                        float(bound[first])))
    assert rel <= helpers.IGEMM_REL_INF_TOL, "%s: rel_inf %.3e > %.1e" % (what, rel, helpers.IGEMM_REL_INF_TOL)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", [c["id"] for c in S.DIRECT_CASES])
def test_direct_case(ops, gpu, case_id):
    q = S.place(case_id, gpu, ops)
    q["run"]()
    torch.cuda.synchronize()
    ref, bound = S.reference(case_id)
    _assert_close(q["out_view"], ref, bound, case_id)
    for g in S.guards(q):
        g.assert_untouched(case_id)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", [c["id"] for c in S.MFMA_CASES])
def test_mfma_case_and_the_direct_kernel_on_the_same_problem(ops, gpu, case_id):
    """the MFMA kernel within the bound, and so is the direct kernel the plans can switch to by policy; the two agree to the suite's tolerance"""
    ref, bound = S.reference(case_id)
    outs = []
    for kernel in ("mfma", "direct"):
        q = S.place(case_id, gpu, ops, kernel=kernel)
        q["run"]()
        torch.cuda.synchronize()
        _assert_close(q["out_view"], ref, bound, "%s (%s kernel)" % (case_id, kernel))
        for g in S.guards(q):
            g.assert_untouched(case_id)
        outs.append(q["out_view"].float().cpu())
    diff = float((outs[0] - outs[1]).abs().max() / outs[1].abs().max().clamp_min(1e-12))
    assert diff <= 1e-3, "%s: MFMA and direct kernels differ by rel_inf %.3e" % (case_id, diff)
    assert bool(((outs[0] - outs[1]).abs().double() <= 2 * bound).all())
