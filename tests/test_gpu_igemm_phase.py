"""The phase form of the implicit GEMM (csrc/igemm.hip: IG_CONV2D_PHASE), pinned by kernel symbol at its tile, phase and border edges,
in the style of tests/test_gpu_igemm_forms.py.

A 3x3 convolution (padding 1) over a nearest x2 up-sampled map touches, per output pixel (2i + a, 2j + b), a 2x2 block of SOURCE
pixels: the nine weights collapse onto four sums that depend on the phase (a, b) only.  The kernel runs the four 2x2 convolutions as
one GEMM whose rows are phase-major and whose tile grid is padded per phase.  Per case:

1. the kernel symbol the launch recorded (ops.Profiler) is the one the case names, and the shape note says "taps4 phase";
2. poisoned surroundings (helpers.Guarded): NaN guard images before and after the batch, lda = Cin + 8 with NaN pad columns, NaN rows
   after W (the four phase blocks), bias and rowvec; outputs at ld = Nout + 16 inside guard rows that must come back bit for bit;
3. two references:
   (i)  fp64 of the phase GEMM over the EXACT fp16 pack: the element-wise bound of helpers.assert_igemm_close with Ktot = 4 Cin --
        derived from the number formats, no slack;
   (ii) fp64 conv2d(nearest x2 (x), w9, padding = 1) from the UNROUNDED fp32 weights: the suite's per-tensor rel_inf <= 2e-3 (what the
        form changes against the 9-tap gather is where the weights are rounded: one rounding of a sum instead of the roundings of
        its terms).
Split-K is refused for this form (the selector answers splitk 1), so there is no split case."""
import pytest
import torch

from helpers import IGEMM_REL_INF_TOL, assert_igemm_close
from igemm_forms import F32, case_policy
from igemm_phase_cases import CASES, GROUPS, make_phase_problem, phase_pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _gemm_launches(prof):
    return [(rec[1], rec[2]) for rec in prof.launches if rec[1].startswith("igemm")]


def _check(P, c, what):
    for nm, gd in (("A", P.A), ("W", P.Wg), ("bias", P.Bg), ("rowvec", P.Rv), ("out", P.O), ("out16", P.Mir)):
        if gd is not None:
            gd.assert_untouched("%s: %s" % (what, nm))
    out = P.O.view.detach().cpu()
    assert_igemm_close(out, P.ref, P.mag, P.Ktot, 1.0, what)
    rel9 = float((out.double() - P.ref9).abs().max() / P.ref9.abs().max())
    print("PHASE-CHECK %-70s rel_inf vs the 3x3 conv of the up-sampled map (fp32 weights) %.2e" % (what, rel9))
    assert rel9 <= IGEMM_REL_INF_TOL, "%s: rel_inf %.3e vs the 9-tap reference" % (what, rel9)
    if P.Mir is not None:
        assert_igemm_close(P.Mir.view.detach().cpu(), P.ref, P.mag, P.Ktot, 1.0, what + " fp16 mirror")


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name.split(":")[0].replace(" ", "_") for c in CASES])
def test_phase_form(ops, gpu, idx):
    c = CASES[idx]
    P = make_phase_problem(ops, gpu, c, seed=idx)
    with case_policy(ops, c):
        with ops.Profiler() as prof:
            ops.igemm(**P.kw)
        torch.cuda.synchronize()
    ran = _gemm_launches(prof)
    print("FORM %-60s ran %s" % (c.name, ran))
    assert len(ran) == 1 and ran[0][0] == c.sym, "%s: expected %s, the dispatcher launched %s" % (c.name, c.sym, ran)
    assert "taps4 phase" in ran[0][1] and "splitk" not in ran[0][1], ran
    _check(P, c, "%s [%s]" % (c.name, c.sym))


@pytest.mark.parametrize("idx", range(len(GROUPS)), ids=[c.name.replace(" ", "_") for c in GROUPS])
def test_group_of_three_is_one_launch_and_bit_identical(ops, gpu, idx):
    """three distinct problems of one shape -- the sibling adapter blocks of a pyramid level -- leave as ONE launch, and every problem is
    computed exactly as it is alone"""
    c = GROUPS[idx]
    Ps = [make_phase_problem(ops, gpu, c, seed=100 + 10 * idx + k) for k in range(3)]
    with case_policy(ops, c):
        alone = []
        for P in Ps:
            ops.igemm(**P.kw)
            torch.cuda.synchronize()
            alone.append((P.O.buf.clone(), P.Mir.buf.clone() if P.Mir is not None else None))
            P.O.view.fill_(float("nan"))                                      # the group has to write every element again
            if P.Mir is not None:
                P.Mir.view.fill_(float("nan"))
        with ops.Profiler() as prof:
            ops.igemm_group([ops.igemm_desc(**P.kw) for P in Ps])
        torch.cuda.synchronize()
    ran = _gemm_launches(prof)
    print("FORM %-60s ran %s" % (c.name, ran))
    assert len(ran) == 1 and ran[0][0] == c.sym and "taps4 phase" in ran[0][1] and ran[0][1].endswith(" x3"), ran
    for k, (P, (o1, m1)) in enumerate(zip(Ps, alone)):
        assert torch.equal(P.O.buf.view(torch.int32 if o1.dtype == F32 else torch.int16), o1.view(torch.int32 if o1.dtype == F32 else torch.int16)), \
            "problem %d of the group differs from its single launch" % k
        if m1 is not None:
            assert torch.equal(P.Mir.buf.view(torch.int16), m1.view(torch.int16)), "problem %d: the fp16 mirror differs from its single launch" % k
        _check(P, c, "%s, problem %d" % (c.name, k))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_device_phase_pack_is_the_fp32_sums_rounded_once(ops, gpu, dt):
    g = torch.Generator().manual_seed(4242)
    w = (torch.randn(16, 64, 3, 3, generator=g) * 0.05).to(dt)
    want = phase_pack(w.float()).half().reshape(4, 16, 4 * 64)
    got = ops.pack_conv_w_phase(w.to(gpu)).cpu()
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "%d of %d packed weights differ" % (int((got != want).sum()), want.numel())
