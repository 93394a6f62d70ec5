"""Element-wise bounds of the sampler launches (csrc/sampler.hip) against their fp64 evaluation, shared by tests/test_gpu_sampler.py and
tests/test_gpu_denoise.py.  Derived from the formats; nothing measured, no slack factor:
    model input:  1/2 ulp_out(ref) + 2 * 2^-24 |ref|                       (the fp32 rounding of c_in, one fp32 product)
    step:         1/2 ulp_out(ref) + 8 * 2^-24 (|A x| + |B| (|u| + |g| (|c| + |u|)))
                  (c - u, the fma into u, B * mg, the fma with A x: five fp32 roundings at most, + the fp32 roundings of A, B, g)"""
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def ulp(ref, dt):
    """spacing of dt's grid at |ref| (fp64 tensor)"""
    p, emin = {F16: (10, -24), BF16: (7, -133), F32: (23, -149)}[dt]
    e = torch.frexp(ref.abs().clamp_min(1e-300))[1].double() - 1
    return torch.exp2((e - p).clamp_min(emin))


def input_bound(ref, dt):
    return 0.5 * ulp(ref, dt) + 2 * 2.0 ** -24 * ref.abs()


def step_bound(ref, dt, A, B, x, u, c, g):
    guided = g.abs() * (c.abs() + u.abs()) if c is not None else torch.zeros_like(u)
    mag = (A * x).abs() + abs(B) * (u.abs() + guided)
    return 0.5 * ulp(ref, dt) + 8 * 2.0 ** -24 * mag


def assert_within(got, ref, bound, what):
    o = got.detach().cpu().double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: non-finite output (a poisoned surrounding reached it)" % what
    err = (o - ref).abs()
    exact = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))      # bound 0: an exact copy
    worst = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), exact).max())
    print("SAMPLER-CHECK %-90s worst err/bound %.3f" % (what, worst))
    assert bool((err <= bound).all()), "%s: %d elements beyond the bound (worst err/bound %.2f)" % (what, int((err > bound).sum()), worst)
