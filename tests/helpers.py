import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, GOLD):
    if p not in sys.path:
        sys.path.insert(0, p)


def load_golden(name):
    return torch.load(os.path.join(GOLD, name), weights_only=False)


def check_digest(t, d, tol, what=""):
    """compare a tensor with a stored digest (tests/golden/make_golden.py): strided samples + sums; returns rel-inf"""
    t = t.detach().float().cpu().contiguous()
    assert list(t.shape) == d["shape"], "%s: shape %s != golden %s" % (what, list(t.shape), d["shape"])
    flat = t.reshape(-1)
    s = flat[::d["step"]][:4096]
    ref = d["samples"]
    denom = max(ref.abs().max().item(), 1e-12)
    err = ((s - ref).abs().max().item()) / denom
    assert err <= tol, "%s: rel_inf %.3e > %.1e" % (what, err, tol)
    # whole-tensor check through the abs-sum (catches errors outside the sampled positions)
    rel_sum = abs(float(flat.double().abs().sum()) - d["abssum"]) / max(d["abssum"], 1e-12)
    assert rel_sum <= max(tol, 1e-6) * 2, "%s: abs-sum differs by %.3e" % (what, rel_sum)
    if "full" in d:
        # the whole tensor is stored: element-by-element rel-inf (supersedes the strided samples)
        full = d["full"].float()
        err = max(err, ((t - full).abs().max().item()) / max(full.abs().max().item(), 1e-12))
        assert err <= tol, "%s: rel_inf over the full tensor %.3e > %.1e" % (what, err, tol)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# Element-wise check of an implicit-GEMM result (tests/test_gpu_igemm_forms.py; self-test: tests/test_igemm_check_host.py)
#
#   out = scale * (A . W^T + bias + rowvec + res),  fp16 operands, fp32 accumulation, compared with an fp64 reference:
#
#   |out - ref| <= (Ktot + 8) * 2^-24 * (|A| . |W|^T + |bias| + |rowvec| + |res|) * max(1, |scale|)
#                  + [fp16 output] 2^-11 * |ref| + 2^-25
#                  + [bf16 output] 2^-8 * |ref|
#
# The first term bounds a length-Ktot fp32 sum in ANY order (+ 8: the epilogue's few extra operations); the others are one
# round-to-nearest of the result (2^-25: half the smallest fp16 subnormal).  Nothing in it is measured; there is no slack factor.
# ---------------------------------------------------------------------------------------------------------------------
IGEMM_REL_INF_TOL = 2e-3          # the suite's per-tensor tolerance (tests/test_gpu_ops.py), asserted beside the bound
IGEMM_REL_INF_TOL_BF16 = 1e-2     # (one bf16 rounding alone is 3.9e-3: the suite's bf16 tolerance)


def igemm_bound(ref, mag, ktot, scale, out_dtype):
    """the element-wise bound above; ref / mag fp64 tensors, scale a float or a per-column fp64 tensor"""
    s = scale.abs().clamp_min(1.0) if torch.is_tensor(scale) else max(1.0, abs(float(scale)))
    b = (ktot + 8) * 2.0 ** -24 * mag.double() * s
    if out_dtype == torch.float16:
        b = b + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    elif out_dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * ref.abs()
    else:
        assert out_dtype == torch.float32, out_dtype
    return b


def assert_igemm_close(out, ref, mag, ktot, scale, what="", extra=None, out_dtype=None):
    """every element of `out` within igemm_bound of the fp64 `ref`, AND the per-tensor rel_inf within the suite's tolerance;
    `extra`: an fp64 tensor added to the bound (a derived term of the caller's, e.g. the lo half of a split mirror); `out_dtype`: the
    format the values were rounded to, when `out` itself is a wider copy.
    Returns (worst |err| / bound, rel_inf)."""
    o = out.detach().cpu()
    dt = out_dtype or o.dtype
    o = o.double()
    ref = ref.double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite outputs (a poisoned pad reached a kept element); first at %s" % (
        what, int((~torch.isfinite(o)).sum()), tuple(int(v) for v in (~torch.isfinite(o)).nonzero()[0]))
    bound = igemm_bound(ref, mag, ktot, scale, dt)
    if extra is not None:
        bound = bound + extra
    err = (o - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    rel = float(err.max() / ref.abs().max().clamp_min(1e-12))
    print("IGEMM-CHECK %-70s worst err/bound %.3f  rel_inf %.2e" % (what, worst, rel))
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()
        first = tuple(int(v) for v in idx[0])
        rows = sorted({int(v) for v in idx[:, 0]})
        raise AssertionError("%s: %d of %d elements beyond the fp32-accumulation bound (worst err/bound %.2f); first at %s: got %.6g want %.6g "
                             "bound %.3g; first-axis indices hit: %s%s" % (what, int(bad.sum()), bad.numel(), worst, first, float(o[first]),
                                                                            float(ref[first]), float(bound[first]), rows[:12], " ..." if len(rows) > 12 else ""))
    tol = IGEMM_REL_INF_TOL_BF16 if dt == torch.bfloat16 else IGEMM_REL_INF_TOL
    assert rel <= tol, "%s: rel_inf %.3e > %.1e" % (what, rel, tol)
    return worst, rel


_POISON = {torch.float16: 1.2345e2, torch.float32: -7.6543e4, torch.bfloat16: 3.5e3, torch.int32: 0x5A5A5A5A}     # fixed, non-NaN


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """An operand or result that lives INSIDE a larger allocation.

    Guarded.out(...)  : an output; the surroundings hold a fixed non-NaN bit pattern and must come back bit for bit.
    Guarded.inp(...)  : an input; the surroundings hold NaN, so anything read from them that reaches a kept accumulator shows
                        (the MFMA propagates NaN) -- and they must not be written either.
    `valid` is a tuple of slices of the full buffer: .view is the tensor the kernel is given (its strides are the buffer's)."""

    def __init__(self, full_shape, valid, dtype, device, fill):
        self.buf = torch.full(tuple(full_shape), fill, dtype=dtype, device=device)
        self.valid = tuple(valid)
        self.view = self.buf[self.valid]
        self.is_input = False
        self._snap = None

    @classmethod
    def out(cls, full_shape, valid, dtype, device):
        g = cls(full_shape, valid, dtype, device, _POISON[dtype])
        g._snap = _bits(g.buf).clone()
        return g

    @classmethod
    def inp(cls, data, before, after, device, fill=float("nan")):
        """`data` placed at offset `before` inside a buffer that extends `after` past it (per axis), the rest = fill"""
        full = [b + s + a for b, s, a in zip(before, data.shape, after)]
        valid = tuple(slice(b, b + s) for b, s in zip(before, data.shape))
        g = cls(full, valid, data.dtype, device, fill)
        g.view.copy_(data)
        g.is_input = True
        g._snap = _bits(g.buf).clone()
        return g

    def assert_untouched(self, what=""):
        """everything outside .view is bit for bit what it was (for an input: the view too)"""
        now, snap = _bits(self.buf), self._snap
        diff = now != snap
        if not self.is_input:
            diff[self.valid] = False
        if bool(diff.any()):
            idx = diff.nonzero()
            raise AssertionError("%s: %d element(s) outside the problem were written; first at buffer index %s (valid region %s of %s)" % (
                what, int(diff.sum()), tuple(int(v) for v in idx[0]), [(s.start, s.stop) for s in self.valid], tuple(self.buf.shape)))



# ---------------------------------------------------------------------------------------------------------------------
# Element-wise check of an attention result (tests/test_gpu_attn_forms.py; self-test: tests/test_attn_check_host.py)
#
#   out[i][d] = sum_j p_ij v_jd / sum_j p_ij,   p_ij = 2^(s_ij - m_i),   s_ij = c * q_i . k_j   (c takes q.k to the exp2 domain;
#   c = 1 when K arrives pre-scaled), compared with an fp64 reference over the SAME fp16 operands.  With w = softmax weights,
#   mag = w . |V|, A_ij = |c| * |q_i| . |k_j| and l_i = sum_j 2^(s_ij - max_j s_ij) >= 1, every kernel of the family obeys
#
#   |out - ref| <=   [score accumulation]  (W_g . |V| + |ref| * rowsum(W_g)) / (1 - rowsum(W_g)),   W_g = w * (2^delta - 1 + 2^-22),
#                                          delta_ij = (D + 8) * 2^-24 * (A_ij + max_j A_ij)
#                  + [P rounded to fp16]   sum_j max(2^-11 * w_ij, 2^-25 / l_i) * |v_jd|            (flash kernels only)
#                  + [fp32 sums of O, l]   2 * (Lk + ceil(Lk / 64) + 8) * 2^-24 * mag
#                  + [fp16 output]         2^-11 * |ref| + 2^-25
#
# score accumulation: s is a length-D fp32 sum in ANY order whose accumulator also carries the reference point m (the folded
#   kernels start the MFMA at -m; the plain ones subtract m in one fma), and m is itself one of the row's scores, so every partial sum is
#   at most A_ij + max_j A_ij in magnitude: (D + 1) roundings, + 7 for c (a rounded fp32 product of two rounded constants) and for the
#   subtraction of the moved reference point.  A score off by delta multiplies p by 2^delta in the numerator AND the denominator: the
#   quotient rule gives the expression above (exact, not first order).  2^-22: v_exp_f32 is good to 1 ulp = 2^-23, taken twice (p, and
#   the rescale factor of a moved reference point).
# P rounded to fp16: only the numerator sees it (l sums the fp32 values): one round-to-nearest of a p that lies anywhere between the
#   smallest subnormal and 2^8 (the deferred reference point), i.e. 2^-11 relative or 2^-25 absolute.  The absolute part is taken
#   against l at the TRUE maximum, where it is largest (a deferred reference point is lower, which scales p up and the error down).
# fp32 sums: O and l each are a length-Lk sum in any order, rescaled at most once per 64-key tile (one rounding each); + 8: the
#   exchange of the half-rows' sums, the reciprocal (1 ulp) and the final product.  |ref| <= mag turns the l part into mag as well.
# fp16 output: one round-to-nearest of the result (2^-25: half the smallest fp16 subnormal).
# Nothing in it is measured; there is no slack factor.
# ---------------------------------------------------------------------------------------------------------------------
ATTN_REL_INF_TOL = 2e-3           # the suite's per-tensor tolerance (tests/test_gpu_ops.py), asserted beside the bound


def attn_reference(q, k, v, c, D=None, p_fp16=True, mask=None):
    """fp64 reference and element-wise bound of softmax_2(c * q k^T) v.  q [N][Lq][D], k, v [N][Lk][D] (N = batch * heads; k, v may
    have N = 1: broadcast), c: float.  mask (bool [Lq][Lk] or [N][Lq][Lk], True = visible; every query sees at least one key): a masked
    weight is exactly 0 and carries no error term, and the largest |q| . |k| is taken over the visible keys.
    Returns (ref, bound), both [N][Lq][D] fp64."""
    q, k, v = q.double(), k.double(), v.double()
    D = D or q.shape[-1]
    Lk = k.shape[-2]
    s = (q @ k.transpose(-1, -2)) * c
    A = (q.abs() @ k.abs().transpose(-1, -2)) * abs(c)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
        A = A.masked_fill(~mask, 0.0)
    smax = s.max(-1, keepdim=True).values
    e = torch.exp2(s - smax)
    l = e.sum(-1, keepdim=True)
    w = e / l
    va = v.abs()
    ref = w @ v
    mag = w @ va
    delta = (D + 8) * 2.0 ** -24 * (A + A.max(-1, keepdim=True).values)
    wg = w * (torch.exp2(delta) - 1 + 2.0 ** -22)
    sg = wg.sum(-1, keepdim=True)
    bound = (wg @ va + ref.abs() * sg) / (1 - sg)
    if p_fp16:
        pr = torch.maximum(2.0 ** -11 * w, 2.0 ** -25 / l)
        if mask is not None:
            pr = pr.masked_fill(~mask, 0.0)
        bound = bound + pr @ va
    bound = bound + 2 * (Lk + (Lk + 63) // 64 + 8) * 2.0 ** -24 * mag
    bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return ref, bound


def assert_attn_close(out, ref, bound, what=""):
    """every element of `out` finite and within `bound` (attn_reference) of the fp64 `ref`, AND the per-tensor rel_inf within the
    suite's tolerance.  Returns (worst |err| / bound, rel_inf)."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite outputs (a poisoned pad reached a kept element); first at %s" % (
        what, int((~torch.isfinite(o)).sum()), tuple(int(v) for v in (~torch.isfinite(o)).nonzero()[0]))
    err = (o - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    rel = float(err.max() / ref.abs().max().clamp_min(1e-12))
    print("ATTN-CHECK %-78s worst err/bound %.3f  rel_inf %.2e" % (what, worst, rel))
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()
        first = tuple(int(v) for v in idx[0])
        rows = sorted({tuple(int(v) for v in r[:-1]) for r in idx[:4096]})
        raise AssertionError("%s: %d of %d elements beyond the format-derived bound (worst err/bound %.2f); first at %s: got %.6g want %.6g "
                             "bound %.3g; rows hit: %s%s" % (what, int(bad.sum()), bad.numel(), worst, first, float(o[first]),
                                                            float(ref[first]), float(bound[first]), rows[:8], " ..." if len(rows) > 8 else ""))
    assert rel <= ATTN_REL_INF_TOL, "%s: rel_inf %.3e > %.1e" % (what, rel, ATTN_REL_INF_TOL)
    return worst, rel


# ---------------------------------------------------------------------------------------------------------------------
# Element-wise check of a fused feed-forward result (tests/test_gpu_ffn_forms.py; self-test: tests/test_ffn_check_host.py)
#
#   out = [blend]( ((x W1h^T + b1h) * gelu_erf(x W1g^T + b1g)) W2^T + b2 + res ),  fp16 operands, fp32 accumulation, the hidden activation
#   rounded to fp16 once, compared with an fp64 reference over the same operands.  The bound follows the kernel's chain
#       accumulation of the pre-activation (non-zero addends only) -> gelu_erf_f's own derived error -> |gelu'| <= 1.13 and the product ->
#       one fp32 and one fp16 rounding of P -> the K = 2048 accumulation -> the AlphaBlender fold -> the rounding of the stored value
#   and is built, term by term, in tests/ffn_forms.py (reference()); nothing in it is measured and there is no slack factor.
# ---------------------------------------------------------------------------------------------------------------------
FFN_REL_INF_TOL = 2e-3            # the suite's per-tensor tolerance (tests/test_gpu_ops.py), asserted beside the bound


def assert_ffn_close(out, ref, bound, what=""):
    """every element of `out` finite and within `bound` (ffn_forms.reference) of the fp64 `ref`, AND the per-tensor rel_inf within the
    suite's tolerance.  Returns (worst |err| / bound, rel_inf)."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), "%s: %d non-finite outputs (a poisoned pad reached a kept element); first at %s" % (
        what, int((~torch.isfinite(o)).sum()), tuple(int(v) for v in (~torch.isfinite(o)).nonzero()[0]))
    err = (o - ref).abs()
    worst = float((err / bound).max())
    rel = float(err.max() / ref.abs().max().clamp_min(1e-12))
    print("FFN-CHECK %-60s worst err/bound %.3f  rel_inf %.2e" % (what, worst, rel))
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()
        first = tuple(int(v) for v in idx[0])
        rows = sorted({int(v) for v in idx[:, 0]})
        cols = sorted({int(v) for v in idx[:, 1]})
        raise AssertionError("%s: %d of %d elements beyond the format-derived bound (worst err/bound %.2f); first at %s: got %.6g want %.6g "
                             "bound %.3g; rows hit: %s%s; columns hit: %s%s" % (
                                 what, int(bad.sum()), bad.numel(), worst, first, float(o[first]), float(ref[first]), float(bound[first]),
                                 rows[:12], " ..." if len(rows) > 12 else "", cols[:12], " ..." if len(cols) > 12 else ""))
    assert rel <= FFN_REL_INF_TOL, "%s: rel_inf %.3e > %.1e" % (what, rel, FFN_REL_INF_TOL)
    return worst, rel
