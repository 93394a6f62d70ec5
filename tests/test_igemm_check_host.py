"""Self-test of the implicit-GEMM checker (tests/helpers.py: assert_igemm_close, Guarded) on the CPU: fp32 stand-ins of the kernel
stay inside the element-wise bound with no exclusions, and every planted fault -- wrong values in one row, and stores one row or one
column past the problem -- fails."""
import pytest
import torch

from helpers import Guarded, assert_igemm_close, igemm_bound

SHAPES = [(65, 80, 32), (129, 336, 96), (257, 320, 2880), (130, 256, 2048)]


def _h(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half().float()


def _problem(M, N, K, res_f32=False, scale=1.0):
    x, w, b = _h((M, K), 1), _h((N, K), 2, 0.05), torch.randn(N, generator=torch.Generator().manual_seed(3))
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(4))
    if not res_f32:
        r = r.half().float()
    ref = (x.double() @ w.double().t() + b.double() + r.double()) * scale
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs() + r.double().abs()
    return x, w, b, r, ref, mag


def _standins(x, w, b, r, scale, K):
    blas = (x @ w.t() + b + r) * scale                                  # fp32 accumulation, the library's order
    seq = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, K, 32):                                          # fp32 accumulation in 32-deep chunks (a k-loop's order)
        seq = seq + x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].t()
    return {"blas": blas, "chunk32": (seq + b + r) * scale}


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("scale,res_f32", [(1.0, False), (0.7, True), (1.5, True)])
def test_fp32_standins_are_inside_the_bound(M, N, K, scale, res_f32):
    x, w, b, r, ref, mag = _problem(M, N, K, res_f32, scale)
    for name, o in _standins(x, w, b, r, scale, K).items():
        for dt in (torch.float16, torch.float32, torch.bfloat16):
            worst, _ = assert_igemm_close(o.to(dt), ref, mag, K, scale, "%s %s %dx%dx%d" % (name, dt, M, N, K))
            assert worst <= 1.0


def test_bound_is_the_stated_formula():
    ref = torch.tensor([[2.0, -3.0]], dtype=torch.float64)
    mag = torch.tensor([[5.0, 7.0]], dtype=torch.float64)
    u = 2.0 ** -24
    assert torch.equal(igemm_bound(ref, mag, 32, 1.0, torch.float32), 40 * u * mag)
    assert torch.equal(igemm_bound(ref, mag, 32, 0.5, torch.float32), 40 * u * mag)               # max(1, |scale|)
    assert torch.equal(igemm_bound(ref, mag, 32, -2.0, torch.float32), 40 * u * mag * 2.0)
    assert torch.equal(igemm_bound(ref, mag, 96, 1.0, torch.float16), 104 * u * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25)
    assert torch.equal(igemm_bound(ref, mag, 96, 1.0, torch.bfloat16), 104 * u * mag + 2.0 ** -8 * ref.abs())


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
def test_planted_value_faults_fail(M, N, K, dt):
    x, w, b, r, ref, mag = _problem(M, N, K)
    good = _standins(x, w, b, r, 1.0, K)["chunk32"]
    dropped = good.clone()
    dropped[M - 1] -= x[M - 1, K - 32:] @ w[:, K - 32:].t()            # the last row misses one 32-deep k-slice
    wrong_res = good.clone()
    wrong_res[M - 1] += r[M - 2] - r[M - 1]                             # the last row took its neighbour's residual
    for name, o in (("dropped k-slice", dropped), ("neighbour's residual", wrong_res)):
        with pytest.raises(AssertionError, match="beyond the fp32-accumulation bound"):
            assert_igemm_close(o.to(dt), ref, mag, K, 1.0, name)


def test_nan_from_a_poisoned_pad_fails():
    x, w, b, r, ref, mag = _problem(65, 80, 32)
    o = _standins(x, w, b, r, 1.0, 32)["blas"].half()
    o[64, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_igemm_close(o, ref, mag, 32, 1.0, "nan")


@pytest.mark.parametrize("dt", [torch.float16, torch.float32, torch.bfloat16])
def test_guarded_output_sees_one_row_and_one_column_overruns(dt):
    M, N = 65, 80
    vals = torch.randn(M, N).to(dt)

    def fresh():
        g = Guarded.out((M + 64, N + 16), (slice(0, M), slice(0, N)), dt, "cpu")
        assert g.view.shape == (M, N) and g.view.stride(0) == N + 16 and not bool(torch.isnan(g.buf.float()).any())
        g.view.copy_(vals)
        return g

    fresh().assert_untouched("clean")
    g = fresh()
    g.buf[M, 5] = vals[0, 5]                                            # a store one row past the problem
    with pytest.raises(AssertionError, match="outside the problem"):
        g.assert_untouched("row overrun")
    g = fresh()
    g.buf[M - 1, N] = vals[0, 0]                                        # a store one column past the problem
    with pytest.raises(AssertionError, match="outside the problem"):
        g.assert_untouched("column overrun")
    g = fresh()
    g.buf[M + 63, N + 15] = 0                                           # the far corner of the guard
    with pytest.raises(AssertionError, match="outside the problem"):
        g.assert_untouched("corner")


def test_guarded_input_is_nan_outside_and_read_only():
    data = torch.randn(3, 7, 9, 32).half()
    g = Guarded.inp(data, (1, 0, 0, 0), (1, 0, 0, 8), "cpu")
    assert g.buf.shape == (5, 7, 9, 40) and torch.equal(g.view, data)
    assert bool(torch.isnan(g.buf[0]).all()) and bool(torch.isnan(g.buf[4]).all()) and bool(torch.isnan(g.buf[1:4, :, :, 32:]).all())
    g.assert_untouched("clean")
    g.view[0, 0, 0, 0] += 1                                             # an input must not be written at all
    with pytest.raises(AssertionError):
        g.assert_untouched("written input")
    t = Guarded.inp(torch.zeros(4, dtype=torch.int32), (0,), (8,), "cpu", fill=0x5A5A5A5A)
    assert t.buf.tolist() == [0] * 4 + [0x5A5A5A5A] * 8
