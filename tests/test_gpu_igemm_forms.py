"""Every kernel form of the implicit GEMM (csrc/igemm.hip), pinned by its kernel symbol, at its tile and k-loop edges.

FORMS below is the record of what the suite covers: one row per kernel form -- the `prof_symbol` string the launch records, how
the dispatcher is brought to it, and the edge cases run on it.  Every case runs inside ops.Profiler() and FAILS (it is not skipped)
when another kernel than its row names ran: a retuned threshold in igemm_select() has to update the table in the same commit.  The table
itself, the edge generators and the construction of a case's operands live in tests/igemm_forms.py, shared with the selection test
that needs no GPU (tests/test_igemm_select_host.py).

Three checks per case:

1. the element-wise bound of tests/helpers.py (assert_igemm_close) against an fp64 CPU reference of
   out = scale * (A . W^T + bias + rowvec + res) -- derived from the number formats, no measured slack -- and, beside it, the
   suite's per-tensor rel_inf <= 2e-3.  The bound covers the LINEAR epilogues only (bias, rowvec, fp16 / fp32 residual, scale,
   scale2 ranges, the fp32 master + fp16 mirror).  The GEGLU and activation epilogues keep the suite's existing tolerance
   (rel_inf <= 2e-3 against an fp32 reference): their fp32 erf / exp is not covered by the derivation.
2. poisoned surroundings (helpers.Guarded): outputs live at ld = Nout + 16 (ld % 8 == 0 keeps the vector epilogue; + 12 where the
   scalar one is the target) with 64 guard rows, prefilled with a fixed non-NaN bit pattern that must come back bit for bit; A lives
   at lda = Cin + 8 with NaN in the pad columns and NaN in 256 rows after row M (conv / temporal: NaN guard images before and after
   the batch); W, bias, rowvec and the residual are followed by NaN rows.  The MFMA propagates NaN, so a finite result proves that
   nothing outside the problem reached a kept accumulator.  No form is allowed to read a pad: nothing is narrowed.
3. split-K: scratch and ticket words sized exactly by the library (ctrl_igemm_splitk_ws_bytes / _ticket_words) with a guard page after
   each.  The ticket words are the CALLER's to zero (include/ctrl_hip.h: the plans zero a pool once per forward; the kernel does not
   reset them), so what is asserted afterwards is the exact arrival count in every word and an untouched guard page.

Rungs of igemm_select() that are not in the table: none.  The tiles listed with both epilogues (IGEMM_TILES: B) take SWAP from
can_swap(); the 256 x 256 / 256 x 320 ring tiles and the other forced tiles exist in the SWAP = true form only (IGEMM_TILES: R).
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_igemm_close
from igemm_forms import (ALL, BF16, CONV, F16, F32, FORMS, ROWS, SPLITK, TEMP, C, Case, Guarded, _gen, _h,  # noqa: F401  (re-exported:
                         attach_splitk, case_policy, make_problem, ring, splitk_variant, wide8)                # test_gpu_igemm_forms_split_up.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o



# ------------------------------------------------------------------------------------------------------------------------------------
# the generic case runner
# ------------------------------------------------------------------------------------------------------------------------------------
def run_case(ops, gpu, sym, c, seed=0):
    P = make_problem(ops, gpu, c, seed)
    A, Wg, Bg, Rv, Rs, O, Mir = P.A, P.Wg, P.Bg, P.Rv, P.Rs, P.O, P.Mir
    M, Nout, Ktot, Lt, lo_off, ref, mag, colscale = P.M, P.Nout, P.Ktot, P.Lt, P.lo_off, P.ref, P.mag, P.colscale
    with case_policy(ops, c):
        if c.splitk:
            attach_splitk(ops, gpu, c, P)
        with ops.Profiler() as prof:
            ops.igemm(pinned=bool(c.pinned), **P.kw)
        torch.cuda.synchronize()
    Ws, Tk, sk, twords = P.Ws, P.Tk, P.sk, P.twords
    # ---- which kernel ran ----
    launches = [(rec[0], rec[1], rec[2]) for rec in prof.launches if rec[0] not in ("fill_zero", "fill")]
    gemm = [l for l in launches if l[1].startswith("igemm")]
    print("FORM %-44s ran %-52s %s" % (c.name, " + ".join(l[1] or l[0] for l in launches), gemm[0][2] if gemm else ""))
    assert len(gemm) == 1 and gemm[0][1] == sym, "%s: expected %s, the dispatcher launched %s" % (c.name, sym, launches)
    tail = [l[0] for l in launches if not l[1].startswith("igemm")]
    if c.splitk == "finish":
        assert tail == ["splitk_finish"] and "in-launch" not in gemm[0][2], (c.name, launches)
    elif c.splitk == "inlaunch":
        assert tail == [] and "in-launch" in gemm[0][2], (c.name, launches)
    else:
        assert tail == [] and "splitk" not in gemm[0][2], (c.name, launches)
    # ---- check 2: the surroundings ----
    what = "%s [%s]" % (c.name, sym)
    for nm, gd in (("A", A), ("W", Wg), ("bias", Bg), ("rowvec", Rv), ("res", Rs), ("out", O), ("out16", Mir), ("splitk_ws", Ws)):
        if gd is not None:
            gd.assert_untouched("%s: %s" % (what, nm))
    if Tk is not None:
        tk = Tk.buf.cpu()
        assert bool((tk[twords:] == 0x5A5A5A5A).all()), "%s: the guard page after the ticket words was written" % what
        per = 5 if sk > 4 else 1
        want = torch.zeros(twords, dtype=torch.int32)
        ngrp = (sk + 3) // 4
        for t in range(twords // per):
            if sk > 4:
                want[t * 5] = ngrp
                for gi in range(ngrp):
                    want[t * 5 + 1 + gi] = min(4, sk - 4 * gi)
            else:
                want[t] = sk
        assert torch.equal(tk[:twords], want), "%s: ticket words %s, expected the arrival counts %s" % (what, tk[:twords].tolist(), want.tolist())
    # ---- check 1: element-wise bound + rel_inf ----
    out = O.view.detach().cpu()
    if Lt:
        refo, mago = (t.reshape(M // Lt, Lt, Nout).permute(0, 2, 1) for t in (ref, mag))
        sco = colscale[None, :, None]
    else:
        refo, mago, sco = ref, mag, colscale[None, :]
    assert_igemm_close(out, refo, mago, Ktot, sco, what)
    if Mir is not None:
        m = Mir.view.detach().cpu()
        assert_igemm_close(m[:, :Nout], ref, mag, Ktot, colscale[None, :], what + " fp16 mirror")
        if lo_off:
            # lo = fp16(x - hi): x - hi is exact in fp32 and |x - hi| <= 2^-11 |x|, so hi + lo misses x by one fp16 rounding of lo:
            # 2^-11 * 2^-11 |x| + 2^-25; x itself obeys the fp32-output bound
            both = m[:, :Nout].double() + m[:, Nout:2 * Nout].double()
            assert_igemm_close(both, ref, mag, Ktot, colscale[None, :], what + " hi + lo", out_dtype=F32, extra=2.0 ** -22 * ref.abs() + 2.0 ** -25)



@pytest.mark.parametrize("idx", range(len(ALL)), ids=[c.name.replace(" ", "_") for _, _, c in ALL])
def test_form(ops, gpu, idx):
    sym, how, c = ALL[idx]
    run_case(ops, gpu, sym, c, seed=idx)


@pytest.mark.parametrize("reduce", ["finish", "inlaunch", "inlaunch_tickets"])
@pytest.mark.parametrize("idx", range(len(SPLITK)), ids=[c.name.replace(" ", "_") for _, c in SPLITK])
def test_splitk_form(ops, gpu, idx, reduce):
    sym, c = SPLITK[idx]
    run_case(ops, gpu, sym, splitk_variant(sym, c, reduce), seed=500 + idx)


def test_geglu_and_activation_forms_keep_the_suite_tolerance(ops, gpu):
    """the M >= 65536 GEGLU branch (256 x 128 x 32 at two workgroups per CU): pinned by symbol, guarded like every other case, but
    compared with the suite's rel_inf tolerance -- the erf of the GEGLU epilogue is outside the bound's derivation"""
    M, K, inner = 65536 + 130, 64, 256
    g = _gen(77)
    x, w, b = _h((M, K), g), _h((2 * inner, K), g, 0.05), torch.randn(2 * inner, generator=g)
    y = x.double() @ w.double().t() + b.double()
    ref = y[:, :inner] * F.gelu(y[:, inner:])
    wp = ops.pack_linear_w(w.to(gpu), geglu=True)
    bp = ops.pack_vec(b.to(gpu), geglu=True)
    A = Guarded.inp(x.half(), (0, 0), (256, 8), gpu)
    O = Guarded.out((M + 64, inner + 16), (slice(0, M), slice(0, inner)), F16, gpu)
    with ops.Profiler() as prof:
        ops.igemm(A.view, K + 8, wp, M, 2 * inner, K, bias=bp, geglu=True, segs=[(O.view, inner + 16, 0, inner, ops.SEG_ROW, 1)])
    syms = [rec[1] for rec in prof.launches if rec[1].startswith("igemm")]
    print("FORM %-44s ran %s" % ("large-M GEGLU", syms))
    assert syms == [ring(256, 128, 32, 4, 2, 3, ROWS)], syms
    A.assert_untouched("geglu A")
    O.assert_untouched("geglu out")
    out = O.view.cpu().double()
    assert bool(torch.isfinite(out).all())
    rel = float((out - ref).abs().max() / ref.abs().max())
    print("PARITY large-M GEGLU rel_inf=%.3e" % rel)
    assert rel <= 2e-3, rel
