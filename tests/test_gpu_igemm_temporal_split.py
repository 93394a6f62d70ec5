"""The operand combination the temporal KL-VAE decoder plan (csrc/plan_vae_tdecoder.cpp) is the first to use, at op level through
ops.igemm: IG_TEMPORAL with t_pad = 1 (a padded operand [F + 2][HW][lda] of ONE group of frames) and a_split = 1 (split [hi | lo] rows
against weights packed twice), an fp32 residual, the AlphaBlender fold, and an fp32 output with a split fp16 mirror.

Checks, as tests/test_gpu_igemm_forms.py: the element-wise fp64 bound of tests/helpers.py and poisoned surroundings (NaN guard frames
before and after the padded operand, NaN pad columns, NaN rows behind W / bias / residual / blend operand; outputs inside a fixed bit
pattern that must come back bit for bit).  The fold adds to the bound, per element (v = the epilogue value before the fold, x = the
blend operand, a = sigmoid(mix)):
  * the GEMM part of the bound is scaled by (1 - a);
  * a itself: rcp(1 + exp2(-mix * log2 e)) -- the rounded product moves exp2 by ln 2 * |mix| * log2 e * 2^-24 <= 2^-23 relative for
    |mix| <= 2, v_exp_f32 and v_rcp_f32 are good to 1 ulp = 2^-23 each, the sum rounds once (2^-24): 7 * 2^-24 relative on a <= 1, and
    1 - a rounds once more: together at most 2^-21 (|x| + |v|);
  * a * x + (1 - a) * v: two products and a sum, 3 * 2^-24 (|x| + |v|).
Shapes: C = 64 and 128 (Cin = 128 / 256) at HW = 120 rows per frame (no tile size divides it: tiles straddle frames), F = 1, 2, 5, on the
ring tiles; under ops.set_igemm_wide(2) the same shapes again (Nout < 256 keeps them on the ring tiles) and C = 256, which the wide
256 x 256 tile takes -- the form the SVD VAE's 256- and 512-channel temporal convs run on."""
import pytest
import torch

from helpers import Guarded, assert_igemm_close

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
TEMP = 2


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _run(ops, gpu, C, Fr, HW, wide, mix_value, seed):
    g = torch.Generator().manual_seed(seed)
    M, Cin, Ktot = Fr * HW, 2 * C, 3 * 2 * C
    a_log = torch.randn(1, Fr + 2, HW, C, generator=g)                     # fp32 values: the lo halves carry signal
    hi = a_log.half()
    lo = (a_log - hi.float()).half()
    a_dev = torch.cat([hi, lo], dim=-1)
    a_val = hi.double() + lo.double()                                      # what the kernel multiplies (exactly)
    a_abs = hi.double().abs() + lo.double().abs()
    w_log = (torch.randn(C, C, 3, generator=g) * 0.05).half().float()
    bias = torch.randn(C, generator=g)
    res = torch.randn(M, C, generator=g)                                   # fp32, not fp16-representable
    bx = torch.randn(M, C, generator=g)
    mix = torch.tensor([mix_value])

    def contract(a, w):
        return sum(a[:, t:t + Fr] @ w[:, :, t].t() for t in range(3)).reshape(M, C)

    v = contract(a_val, w_log.double()) + bias.double()[None, :] + res.double()
    vmag = contract(a_abs, w_log.double().abs()) + bias.double().abs()[None, :] + res.double().abs()
    al = torch.sigmoid(mix.double())
    ref = al * bx.double() + (1 - al) * v
    mag = (1 - al) * vmag
    extra = (2.0 ** -21 + 3 * 2.0 ** -24) * (bx.double().abs() + v.abs())

    A = Guarded.inp(a_dev, (1, 0, 0, 0), (1, 0, 0, 8), gpu)
    Wg = Guarded.inp(ops.pack_conv_w_dup(w_log.view(C, C, 3, 1, 1).to(gpu)).cpu(), (0, 0), (64, 0), gpu)
    Bg = Guarded.inp(bias, (0,), (64,), gpu)
    Rs = Guarded.inp(res, (0, 0), (64, 8), gpu)
    Bx = Guarded.inp(bx, (0, 0), (64, 8), gpu)
    Mx = Guarded.inp(mix, (0,), (8,), gpu)
    O = Guarded.out((M + 64, C + 16), (slice(0, M), slice(0, C)), F32, gpu)
    ld16 = 2 * C + 16
    Mir = Guarded.out((M + 64, ld16), (slice(0, M), slice(0, 2 * C)), F16, gpu)
    ops.set_igemm_wide(wide)
    try:
        with ops.Profiler() as prof:
            ops.igemm(A=A.view, lda=Cin + 8, W=Wg.view, M=M, Nout=C, Cin=Cin, taps=3, mode=TEMP, bias=Bg.view, rows_per_img=HW,
                      res=Rs.view, ldres=C + 8, scale=1.0, segs=[(O.view, C + 16, 0, C, ops.SEG_ROW, 1)], F=Fr, HW=HW, out16=Mir.view,
                      ld16=ld16, out16_lo_off=C, blend_mix=Mx.view, blend_x=Bx.view, ld_blend=C + 8, a_split=1, t_pad=True)
        torch.cuda.synchronize()
    finally:
        ops.set_igemm_wide(-1)
    syms = [rec[1] for rec in prof.launches if rec[1].startswith("igemm")]
    what = "temporal t_pad split C%d F%d wide%d [%s]" % (C, Fr, wide, syms[0] if syms else "?")
    assert len(syms) == 1, prof.launches
    for nm, gd in (("A", A), ("W", Wg), ("bias", Bg), ("res", Rs), ("blend_x", Bx), ("mix", Mx), ("out", O), ("out16", Mir)):
        gd.assert_untouched("%s: %s" % (what, nm))
    assert_igemm_close(O.view.detach().cpu(), ref, mag, Ktot, 1.0, what, extra=extra)
    m = Mir.view.detach().cpu()
    assert_igemm_close(m[:, :C], ref, mag, Ktot, 1.0, what + " fp16 mirror", extra=extra)
    both = m[:, :C].double() + m[:, C:2 * C].double()
    # hi + lo misses the fp32 value by one fp16 rounding of lo: 2^-22 |x| + 2^-25
    assert_igemm_close(both, ref, mag, Ktot, 1.0, what + " hi + lo", out_dtype=F32, extra=extra + 2.0 ** -22 * ref.abs() + 2.0 ** -25)
    return syms[0]


@pytest.mark.parametrize("Fr", [1, 2, 5])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("wide", [-1, 2], ids=["default", "wide2"])
def test_temporal_tpad_split_res_blend_mirror(ops, gpu, wide, C, Fr):
    sym = _run(ops, gpu, C, Fr, 120, wide, (-1.5, 0.5, 2.0)[Fr % 3], seed=1000 * C + 10 * Fr + (wide > 0))
    assert sym.startswith("igemm_kernel<") and sym.split(",")[6].strip() == str(TEMP), sym      # a ring tile in the temporal gather


@pytest.mark.parametrize("Fr", [1, 2, 5])
def test_temporal_tpad_split_res_blend_mirror_on_the_wide_tile(ops, gpu, Fr):
    sym = _run(ops, gpu, 256, Fr, 120, 2, (-1.5, 0.5, 2.0)[Fr % 3], seed=7000 + Fr)
    assert sym == "igemm8_kernel<4, %d>" % TEMP, sym
