"""The fused GEGLU feed-forward (csrc/ffn.hip) at its edges, on the GPU: every case of tests/ffn_forms.py against the fp64 reference and the
format-derived bound, operands inside poisoned guards; the small-M schedules, the grouped launch the plans use, and the range check of the
hidden activation.  The checker itself is tested on the host (tests/test_ffn_check_host.py)."""
import pytest
import torch

import helpers
import ffn_forms as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _launch(ops, desc):
    import ctypes as C
    from ctrl_adapter_amd import _lib as L
    L.check(L.lib().ctrl_op_ffn(C.byref(desc), L.cur_stream()))


def _check_outputs(case_id, pair, what):
    """the master and the mirror of one output set within the bound; returns the worst err / bound"""
    c = F.CASE_BY_ID[case_id]
    ref, b32, b16 = F.reference(case_id)
    out, mir = pair
    worst, _ = helpers.assert_ffn_close(out.view, ref, b32 if F.FORMS[c["form"]]["out"] == torch.float32 else b16, what)
    if mir is not None:
        w2, _ = helpers.assert_ffn_close(mir.view, ref, b16, what + " mirror")
        # the mirror is rounded from the fp32 value that was stored
        assert torch.equal(mir.view, out.view.half()), what + ": the fp16 mirror is not the rounded master"
        worst = max(worst, w2)
    return worst


def test_packs_equal_their_host_restatement(ops, gpu):
    """ffn_pack_w2 (and the GEGLU packs of W1 / b1) bit for bit what tests/ffn_forms.py restates from the kernel's comment"""
    g = torch.Generator().manual_seed(1)
    w2 = torch.randn(F.D, F.H, generator=g).half()
    w1 = torch.randn(2 * F.H, F.D, generator=g).half()
    b1 = torch.randn(2 * F.H, generator=g)
    got = ops.ffn_pack_w2(ops.pack_linear_w(w2.to(gpu)))
    assert torch.equal(got.cpu().view(-1), F.pack_w2(w2).reshape(-1))
    assert torch.equal(ops.pack_linear_w(w1.to(gpu), geglu=True).cpu(), F.pack_w1(w1))
    assert torch.equal(ops.pack_vec(b1.to(gpu), geglu=True).cpu(), b1[F.geglu_pack_rows()])


@pytest.mark.parametrize("case_id", [c["id"] for c in F.CASES])
def test_ffn_case(ops, gpu, case_id):
    """finite, every element within the bound, rel_inf within the suite's tolerance, guards untouched (outputs: pad rows before and after
    and pad columns; X inside NaN rows; W1, b1 and the W2 pack inside NaN with the allocation ending where chunk 15's last piece ends)"""
    q = F.place(case_id, gpu, ops)
    _launch(ops, q["descs"][0])
    torch.cuda.synchronize()
    worst = _check_outputs(case_id, q["outs"][0], case_id)
    for g in F.guards(q):
        g.assert_untouched(case_id)
    print("FFN-WORST %s %s %.3f" % (q["case"]["kind"], case_id, worst))


@pytest.mark.parametrize("M", [1, 129, 257])
def test_small_m_schedules_are_bit_identical(ops, gpu, M):
    """CTRL_FF_FUSED=bulk (the first schedule, kept for A/B runs) and =jitter (uneven wave timing) against the default schedule at one
    row, one row past a tile and one row past two tiles: the same bits, three rounds of jitter"""
    ids = [c["id"] for c in F.CASES if c["M"] == M]
    for case_id in ids:
        q = F.place(case_id, gpu, ops, outputs=2)
        _launch(ops, q["descs"][0])
        torch.cuda.synchronize()
        base = [t.buf.clone() for t in q["outs"][0] if t is not None]
        for pol, rounds in (("bulk", 1), ("jitter", 3)):
            prev = ops.set_policy("CTRL_FF_FUSED", pol)
            try:
                for _ in range(rounds):
                    for t in q["outs"][1]:
                        if t is not None:
                            t.buf.copy_(torch.full_like(t.buf, helpers._POISON[t.buf.dtype]))
                    _launch(ops, q["descs"][1])
                    torch.cuda.synchronize()
            finally:
                ops.set_policy("CTRL_FF_FUSED", prev)
            got = [t.buf for t in q["outs"][1] if t is not None]
            for a, b in zip(base, got):
                assert torch.equal(helpers._bits(a), helpers._bits(b)), "%s: CTRL_FF_FUSED=%s differs from the default schedule" % (case_id, pol)
        for g in F.guards(q):
            g.assert_untouched(case_id)


@pytest.mark.parametrize("M,n", [(127, 2), (127, 3), (127, 4), (1153, 2), (1153, 3), (1153, 4)])
def test_grouped_launch(ops, gpu, M, n):
    """op_ffn_fused_group with n > 1, the form the video adapter runs (outside a plan only ctrl_op_ffn_group reaches it): members with
    different weights, epilogue forms and strides in ONE launch; at M = 127 `per` = 8, so seven idle workgroups sit between members.
    Every member bit-identical to its single launch and within the bound, all guards untouched, one ffn_fused launch `x<n>`."""
    ids = [c["id"] for c in F.CASES if c["M"] == M]
    ids = ids[:n] if n < 4 else ids[-4:]
    assert len({F.CASE_BY_ID[i]["form"] for i in ids}) >= 2 and len({F.CASE_BY_ID[i]["stride"] for i in ids}) >= 2
    qs = [F.place(i, gpu, ops, outputs=2) for i in ids]
    for q in qs:
        _launch(ops, q["descs"][0])
    with ops.Profiler() as prof:
        ops.ffn_group([q["descs"][1] for q in qs])
    torch.cuda.synchronize()
    ff = [l for l in prof.launches if l[0] == "ffn_fused"]
    assert len(ff) == 1 and ff[0][2].endswith(" x%d" % n), prof.launches
    per = (((M + 127) // 128) + 7) // 8 * 8
    assert ff[0][6] == per * n * 512, (ff[0][6], per, n)
    for i, q in zip(ids, qs):
        for a, b in zip(q["outs"][0], q["outs"][1]):
            if a is not None:
                assert torch.equal(helpers._bits(a.buf), helpers._bits(b.buf)), "%s: member differs from its single launch" % i
        _check_outputs(i, q["outs"][1], "group x%d %s" % (n, i))
        for g in F.guards(q):
            g.assert_untouched(i)


def _range_problem(M, gpu, ops, b1h, b1g, w1h_col0=0.0):
    """W2 = 0 (finite outputs whatever P is), W1 = 0 but for column 0 of the hidden half, x[:, 0] = 1: h = b1h + w1h_col0, g = b1g on the
    real rows, h = b1h on the zero-filled rows beyond M.  X sits inside NaN rows."""
    x = torch.zeros(M, F.D, dtype=torch.float16)
    x[:, 0] = 1.0
    w1 = torch.zeros(2 * F.H, F.D, dtype=torch.float16)
    w1[:F.H, 0] = w1h_col0
    b1 = torch.cat([torch.full((F.H,), float(b1h)), torch.full((F.H,), float(b1g))])
    xg = helpers.Guarded.inp(x, (F.PAD_ROWS, 0), (F.PAD_ROWS, 0), gpu)
    w1p, b1p = F.pack_w1(w1).to(gpu), b1[F.geglu_pack_rows()].to(gpu)
    w2p = torch.zeros(4, F.D, 512, dtype=torch.float16, device=gpu)
    out = helpers.Guarded.out((M + 2 * F.PAD_ROWS, F.D), (slice(F.PAD_ROWS, F.PAD_ROWS + M), slice(0, F.D)), torch.float16, gpu)
    return xg, out, ops.ffn_desc(xg.view, w1p, b1p, w2p, out.view), (w1p, b1p, w2p)


def test_range_check_of_the_hidden_activation(ops, gpu):
    """ctrl_range_check(1) on the hidden activation P (W2 = 0 throughout, so nothing but P can raise the flag while P is finite in fp16):
      * P = 255.8984375 * gelu(256) = 65510 on real rows: beyond 65504, yet rounded to the finite 65504 -- the flag is raised and the
        outputs are finite (0); only the flag tells.  P = 300 * gelu(300) = 9e4 rounds to inf, and 0 * inf is NaN: flag raised as well
      * the same operands scaled into range (P = 4e4) raise nothing
      * P = 0 on every row that exists and 9e4 only on the zero-filled rows beyond M (M = 1, 129, 193) raises nothing: the check looks at
        the rows that exist; one real row among them out of range is seen
      * X sits inside NaN rows throughout, which raise nothing either; with the check off nothing is recorded."""
    from ctrl_adapter_amd import _lib as L
    lib = L.lib()
    assert lib.ctrl_range_check(0) == 0 and lib.ctrl_range_status(1) == 2
    keep = []

    def run(M, b1h, b1g, col0=0.0, finite=True, edit=None):
        xg, out, d, w = _range_problem(M, gpu, ops, b1h, b1g, col0)
        keep.append((xg, out, d, w))
        if edit:
            edit(xg)
            xg._snap = helpers._bits(xg.buf).clone()
        _launch(ops, d)
        torch.cuda.synchronize()
        if finite:
            assert bool(torch.isfinite(out.view).all()) and float(out.view.abs().max()) == 0.0
        out.assert_untouched("range M%d" % M)
        xg.assert_untouched("range M%d" % M)

    run(129, 300.0, 300.0, finite=False)                       # off: nothing is recorded
    assert lib.ctrl_range_check(1) == 1
    try:
        assert lib.ctrl_range_status(1) == 0
        for M in (1, 128, 129):
            run(M, 65510.0 / 256.0, 256.0)                     # 65510 on real rows: out of range, finite once rounded
            assert lib.ctrl_range_status(1) == 1 and lib.ctrl_range_status(1) == 0, M
            run(M, 300.0, 300.0, finite=False)                 # 9e4 on real rows
            assert lib.ctrl_range_status(1) == 1 and lib.ctrl_range_status(1) == 0, M
            run(M, 200.0, 200.0)                               # the same operands scaled into range: 4e4
            assert lib.ctrl_range_status(1) == 0, M
        for M in (1, 129, 129 + 64):                           # (193: the last tile's second wave row holds one real row; 129: none)
            run(M, 300.0, 300.0, -300.0)                       # h = 0 on the rows that exist, 300 on the zero-filled ones
            assert lib.ctrl_range_status(1) == 0, "M %d: a row beyond M raised the range flag" % M

        def last_row_out_of_range(xg):
            xg.view[128, 0] = 0.0
        run(129, 300.0, 300.0, -300.0, finite=False, edit=last_row_out_of_range)      # one real row out of range, alone in the last tile
        assert lib.ctrl_range_status(1) == 1
    finally:
        lib.ctrl_range_check(0)
