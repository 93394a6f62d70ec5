"""The fused GEGLU feed-forward (csrc/ffn.hip) at its edges: case table, problem builder, fp64 reference, element-wise bound, an fp32
emulation of the kernel's arithmetic and the planted errors the bound has to reject.

    GPU tests: tests/test_gpu_ffn_forms.py        host self-test (no GPU): tests/test_ffn_check_host.py

The op.   y = x W1^T + b1 (K = 512; hidden half h = y[:, :2048], gate half g = y[:, 2048:]),  P = h * gelu_erf(g),
          z = P W2^T + b2 + res (K = 2048),  out = z or the AlphaBlender fold (1 - a) z + a blend_x,  a = sigmoid(mix);
          out is stored as fp32 or fp16, the optional fp16 mirror is rounded from the fp32 value.

The kernel computes   y^ = fp32(x W1^T + b1)            an fp32 sum in some order, the bias rides in the accumulator
                      P^ = fp16(fp32(h^ * gelu_erf_f(g^)))
                      z^ = fp32(P^ W2^T + b2 + res)
and the bound follows that chain with u = 2^-24 (one round-to-nearest in fp32); every term is derived, none is measured:

  dy   accumulation of y:  (n - 1) u mag_y,  mag_y = |x| |W1|^T + |b1|,  n = the NON-ZERO addends of the element (products and bias):
       adding an exact zero rounds nothing, so a sum of n non-zero terms takes n - 1 roundings whatever the order, each of a partial sum
       that is at most mag_y.  One-hot rows (n <= 1) therefore have an EXACT pre-activation: what pins the activation itself in the
       `gate` cases.  The dense cases use the plain any-order form of the implicit-GEMM bound, (K + 8) u mag_y.
  eg   gelu_erf_f (csrc/common.h) against the exact GELU:  eg(g) = C_G |g| + u |gelu(g)|,  C_G = 9.4e-7 (GELU_C below, term by term)
  dP   P^ against P = h gelu(g):   dP0 = |gelu(g)| dh + (|h| + dh) (1.13 dg + eg(|g| + dg))          (|gelu'| <= 1.13)
                                   dP  = dP0 + (2^-11 + 2^-24 + 2^-35) (|P| + dP0) + 2^-25
       = propagation through GELU and the product, one fp32 rounding of the product, one fp16 rounding of the rounded product
       (2^-35: the fp16 rounding acts on the fp32-rounded value), 2^-25 = half the smallest fp16 subnormal.
  dz   dP |W2|^T + (n2 - 1) u mag_z,  mag_z = (|P| + dP) |W2|^T + |b2| + |res|,  n2 = the non-zero addends (products, bias, residual);
       dense: (2048 + 8) u mag_z.
  blend  a^ = rcp(1 + exp(-mix)) is good to rho_a = (5 + |mix|) u relative: the product mix * log2(e) in front of v_exp_f32 (|mix| u on
       the result), v_exp_f32 and v_rcp_f32 at one ulp = 2 u each, the addition u.  With z^ = z +- dz:
         d = (1 - a) dz + rho_a a (|blend_x| + |z| + dz) + u (1 - a) (|z| + dz) + 2 u (a |blend_x| + (1 - a) (|z| + dz))
       (the error of a^ on both operands, the rounding of 1 - a^, two products and one sum).
  store  fp32: nothing more.  fp16 (output or mirror): + 2^-11 (|ref| + d) + 2^-25.
"""
import functools
import itertools
import math

import torch

U = 2.0 ** -24
D, H, HC, NCH = 512, 2048, 128, 16          # dim, hidden, hidden units per chunk, chunks (csrc/ffn.hip: namespace ff)

# ---------------------------------------------------------------------------------------------------------------------------
# gelu_erf_f (csrc/common.h):   t = rcp(fma(|x|, p', 1)),  e = exp2(x x c'),  hp = t (c1 + t (c2 + t (c3 + t (c4 + t c5)))),  c_k = a_k / 2,
#                               result = fma(-|x| hp, e, max(x, 0))
# against gelu(x) = max(x, 0) - |x| (P(t) / 2) e^(-x^2 / 2) + |x| eps(z) / 2,  z = |x| / sqrt 2.  Every term is a bound on |error| / |x|:
#   AS      Abramowitz-Stegun 7.1.26: |eps| <= 1.5e-7 on erf, half of it on the tail product                              0.75e-7
#   T       t carries a relative error rho_t <= u (p' = the rounded product of two constants) + u (the fma) + 2 u (v_rcp_f32, 1 ulp)
#           = 4 u; the tail answers with |t hp'(t)| e(t) rho_t, and sup_t |sum_k k c_k t^k| e(t) = GELU_SENS_T (taken at t = 1,
#           where e = 1; the host self-test evaluates the supremum on a grid)                                              1.73 * 4 u
#   HORNER  nine roundings at most (five products and four sums when nothing is contracted into an fma), each of an intermediate
#           q5 = c5 t, s4 = c4 + q5, q4 = t s4, ..., hp whose magnitudes are at most .531 .727 .727 .711 .711 .569 .569 .70 .50 on
#           0 < t <= 1 (the self-test evaluates them), and every later step multiplies by t <= 1: sum = GELU_SUM_HORNER       5.75 u
#   EXP     e = v_exp_f32 (1 ulp = 2 u) of an argument with two roundings (x x, times c') and a rounded constant: 3 u relative on an
#           argument a, i.e. 3 u a ln 2 on e; a 2^-a ln 2 <= 1 / e = 0.37, and e multiplies hp <= 1 / 2                 (2 + 3 * 0.37) u / 2
#   FMA     the product |x| hp rounds once (u on a factor <= 1 / 2); the fma itself rounds the RESULT: u |gelu(x)|, the second
#           term of eg                                                                                                      u / 2
# The host self-test also checks the floor: an fp32 emulation with exact rcp and exp2 reaches 2.8e-7 |x| on [-12, 12].
# ---------------------------------------------------------------------------------------------------------------------------
GELU_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
GELU_P = 0.3275911
GELU_SENS_T = 1.73
GELU_SUM_HORNER = 5.75
GELU_TERMS = (("AS", 0.75e-7), ("T", GELU_SENS_T * 4 * U), ("HORNER", GELU_SUM_HORNER * U), ("EXP", (2 + 3 * 0.37) * U / 2), ("FMA", U / 2))
GELU_C = sum(v for _, v in GELU_TERMS)
GELU_SLOPE = 1.13


def gelu64(g):
    return 0.5 * g * (1.0 + torch.special.erf(g / math.sqrt(2.0)))


def gelu_err(g_abs, gelu_abs):
    """eg above: the derived bound on |gelu_erf_f(g) - gelu(g)|"""
    return GELU_C * g_abs + U * gelu_abs


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def gelu_erf_f_emul(x, act="erf"):
    """fp32 restatement of gelu_erf_f, operation by operation (rcp and exp2 correctly rounded, nothing contracted); act = "tanh" /
    "quick": the approximations a wrong kernel might use instead (planted errors)"""
    x = x.float()
    if act == "tanh":
        return (0.5 * x.double() * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x.double() + 0.044715 * x.double() ** 3)))).float()
    if act == "quick":
        return (x.double() * torch.sigmoid(1.702 * x.double())).float()
    ax = x.abs()
    pk = _f32(GELU_P) * _f32(0.70710678118654752)
    t = 1.0 / (ax * pk + 1.0)
    e = torch.exp2(x * x * (_f32(-0.5) * _f32(1.4426950408889634)))
    c = [_f32(0.5) * _f32(a) for a in GELU_A]
    hp = t * (c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * c[4]))))
    return (-ax * hp) * e + x.clamp_min(0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# The case table
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("dense", "sparse", "gate")
MS = (1, 16, 127, 128, 129, 255, 257, 1153)          # ntm = 1, 1, 1, 1, 2, 2, 3, 10


def m_class(M):
    return "below a tile" if M < 128 else "one full tile" if M == 128 else "ragged tiles" if M < 1000 else "ten tiles"


# epilogue forms: (residual dtype, output dtype, fp16 mirror, bias, AlphaBlender fold)
FORMS = {
    "f32": dict(res=torch.float32, out=torch.float32, mirror=True, bias=True, blend=False),       # the fp32 stream: master + mirror
    "f16": dict(res=torch.float16, out=torch.float16, mirror=False, bias=True, blend=False),      # the fp16 token stream
    "plain": dict(res=None, out=torch.float16, mirror=False, bias=False, blend=False),            # the epilogue's packed fp16 path
    "bias": dict(res=None, out=torch.float32, mirror=False, bias=True, blend=False),
    "blend": dict(res=torch.float32, out=torch.float32, mirror=True, bias=True, blend=True),      # the temporal block's feed-forward
}
# row strides (ld of the output, ldres, ld16; the AlphaBlender operand rides on ldres'): all 512, and each one larger on its own
STRIDES = {"all512": (512, 512, 512), "ld": (520, 512, 512), "ldres": (512, 536, 512), "ld16": (512, 512, 528)}


def stride_matters(form, stride):
    f = FORMS[form]
    return stride in ("all512", "ld") or (stride == "ldres" and f["res"] is not None) or (stride == "ld16" and f["mirror"])


def _table():
    forms = list(FORMS)
    cases = []
    seen_stride = {}
    for ki, kind in enumerate(KINDS):
        for mi, M in enumerate(MS):
            form = forms[(mi + 2 * ki) % len(forms)]
            ok = [s for s in STRIDES if stride_matters(form, s)]
            n = seen_stride.get((kind, form), 0)
            seen_stride[(kind, form)] = n + 1
            cases.append((kind, M, form, ok[(mi + n + ki) % len(ok)]))
    # what the walk above leaves out of M class x form, and a fourth member for the groups of one row tile
    cases += [("sparse", 128, "f16", "ldres"), ("gate", 128, "blend", "ld16"), ("gate", 1153, "f32", "ldres"), ("sparse", 1153, "bias", "ld"),
              ("dense", 127, "f32", "ld16"), ("dense", 16, "blend", "ldres"), ("sparse", 129, "f32", "ld16"), ("gate", 257, "f16", "ldres"),
              ("dense", 255, "f16", "ldres"), ("gate", 1, "f32", "ld16"), ("sparse", 255, "blend", "ld16")]
    return [dict(id="%s-M%d-%s-%s" % c, kind=c[0], M=c[1], form=c[2], stride=c[3], seed=9000 + 17 * i) for i, c in enumerate(cases)]


CASES = _table()
CASE_BY_ID = {c["id"]: c for c in CASES}


def _rnd16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


def sparse_w2_units(n):
    """the four hidden units output channel n reads in the `sparse` / `gate` cases: unit 512 j + (n ^ m_j).  n -> n ^ m_j is a bijection
    of [0, 512), so the 2048 (n, j) pairs hit every hidden unit exactly once; the four units of a channel lie in four different chunks
    (4 j + (n ^ m_j) // 128), and m_j flips bits 4 and 1 of the unit's index, the two bits that select its k-step inside a chunk
    (csrc/ffn.hip: ffn_pack_w2_kernel), so they lie in four different k-steps"""
    return [512 * j + (n ^ m) for j, m in enumerate((0, 0b10, 0b10000, 0b10010))]


def unit_kstep(u):
    """k-step (0..3) of hidden unit u inside its chunk: u % 128 = 32 q' + 16 (kap >> 1) + 4 q + 2 (kap & 1) + i"""
    return 2 * ((u >> 4) & 1) + ((u >> 1) & 1)


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """the operands of a case, on the CPU: x fp16 [M][512], w1 fp16 [4096][512] (rows 0..2047 hidden, 2048.. gate), b1 fp32 [4096],
    w2 fp16 [512][2048], b2 fp32 [512] | None, res [M][512] | None, blend_x / mix | None"""
    c = CASE_BY_ID[case_id]
    kind, M, f = c["kind"], c["M"], FORMS[c["form"]]
    g = torch.Generator().manual_seed(c["seed"])
    p = dict(case=c)
    if kind == "dense":
        p["x"] = _rnd16(g, M, D)
        p["w1"], p["b1"] = _rnd16(g, 2 * H, D, scale=0.03), _rnd16(g, 2 * H, scale=0.1).float()
        p["w2"] = _rnd16(g, D, H, scale=0.03)
    elif kind == "sparse":
        p["x"] = _rnd16(g, M, D)
        w1 = torch.zeros(2 * H, D, dtype=torch.float16)
        rows = torch.arange(2 * H)
        for j in range(3):          # three non-zeros per unit and half, in k-tiles (row + 3 j) % 8: every k-tile over the rows
            k = 64 * ((rows + 3 * j) % 8) + torch.randint(0, 64, (2 * H,), generator=g)
            w1[rows, k] = _rnd16(g, 2 * H, scale=0.5)
        p["w1"], p["b1"] = w1, _rnd16(g, 2 * H, scale=0.1).float()
        w2 = torch.zeros(D, H, dtype=torch.float16)
        for n in range(D):
            v = torch.randn(4, generator=g)
            w2[n, sparse_w2_units(n)] = (torch.sign(v) * (0.25 + 0.5 * v.abs())).half()          # never zero
        p["w2"] = w2
    else:
        # hidden half exactly 1; gate u = x[:, k_u] * (+-2^e): the pre-activation is exact, P = gelu(g) rounded to fp16
        p["x"] = ((torch.rand(M, D, generator=g) * 12.0 - 6.0)).half()
        w1 = torch.zeros(2 * H, D, dtype=torch.float16)
        u = torch.arange(H)
        sign = torch.where(torch.randint(0, 2, (H,), generator=g) == 0, -1.0, 1.0)
        w1[H + u, (u * 7 + 3) % D] = (sign * 2.0 ** (torch.randint(0, 4, (H,), generator=g) - 2.0)).half()
        b1 = torch.zeros(2 * H)
        b1[:H] = 1.0
        p["w1"], p["b1"] = w1, b1
        w2 = torch.zeros(D, H, dtype=torch.float16)
        for n in range(D):          # four unit weights (even channels) or one (odd channels)
            us = sparse_w2_units(n)
            w2[n, us if n % 2 == 0 else us[(n // 2) % 4]] = 1.0
        p["w2"] = w2
    p["b2"] = _rnd16(g, D, scale=0.1).float() if f["bias"] else None
    if f["res"] is None:
        p["res"] = None
    else:
        r = torch.randn(M, D, generator=g)          # the fp32 stream is NOT fp16-representable
        p["res"] = r if f["res"] == torch.float32 else r.half()
    if f["blend"]:
        bx = torch.randn(M, D, generator=g)
        p["blend_x"] = bx if kind != "sparse" else bx.half()
        p["mix"] = torch.tensor([0.3 if kind != "gate" else -0.8])
    else:
        p["blend_x"] = p["mix"] = None
    return p


def _nonzero_count(a, b):
    return (a != 0).float() @ (b != 0).float().t()


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(ref, bound32, bound16): the fp64 reference of the case and the element-wise bounds of the header for a value stored as fp32 and
    as fp16, all fp64 [M][512]"""
    p = problem(case_id)
    dense = p["case"]["kind"] == "dense"
    x, w1, b1, w2 = p["x"].double(), p["w1"].double(), p["b1"].double(), p["w2"].double()
    y = x @ w1.t() + b1
    mag_y = x.abs() @ w1.abs().t() + b1.abs()
    if dense:
        dy = (D + 8) * U * mag_y
    else:
        dy = (_nonzero_count(p["x"], p["w1"]).double() + (b1 != 0).double() - 1).clamp_min(0) * U * mag_y
    h, g, dh, dg = y[:, :H], y[:, H:], dy[:, :H], dy[:, H:]
    gel = gelu64(g)
    P = h * gel
    eg = gelu_err(g.abs() + dg, gel.abs() + GELU_SLOPE * dg)
    dP0 = gel.abs() * dh + (h.abs() + dh) * (GELU_SLOPE * dg + eg)
    dP = dP0 + (2.0 ** -11 + 2.0 ** -24 + 2.0 ** -35) * (P.abs() + dP0) + 2.0 ** -25
    z = P @ w2.t()
    mag_z = (P.abs() + dP) @ w2.abs().t()
    n2 = _nonzero_count(P.float(), p["w2"]).double()
    for t in (p["b2"], p["res"]):
        if t is not None:
            z = z + t.double()
            mag_z = mag_z + t.double().abs()
            n2 = n2 + (t != 0).double()
    acc2 = (H + 8) if dense else (n2 - 1).clamp_min(0)
    d = dP @ w2.abs().t() + acc2 * U * mag_z
    ref = z
    if p["mix"] is not None:
        mix = float(p["mix"][0])
        a = 1.0 / (1.0 + math.exp(-mix))
        rho_a = (5 + abs(mix)) * U
        bx = p["blend_x"].double()
        zz = z.abs() + d
        ref = (1 - a) * z + a * bx
        d = (1 - a) * d + rho_a * a * (bx.abs() + zz) + U * (1 - a) * zz + 2 * U * (a * bx.abs() + (1 - a) * zz)
    return ref, d, d + 2.0 ** -11 * (ref.abs() + d) + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's arithmetic, with the errors a wrong kernel would make (tests/test_ffn_check_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
PLANTED = ("swap_w2_units", "drop_unit", "swap_hidden_gate_fragment", "b1_of_next_chunk", "last_tile_rows_shifted", "tanh_gelu", "p_not_fp16")
# which case kinds must reject which planted error.  `gate` has the same b1 in every chunk, so a bias from the neighbouring chunk cannot
# show there; a dense random case cannot tell tanh from erf, which is what `gate` is for (`sparse` happens to, by 5x and more, but only
# `gate`, whose pre-activation is exact, is required to)
MUST_REJECT = {
    "swap_w2_units": ("dense", "sparse", "gate"),
    "drop_unit": ("dense", "sparse", "gate"),
    "swap_hidden_gate_fragment": ("dense", "sparse", "gate"),
    "b1_of_next_chunk": ("dense", "sparse"),
    "last_tile_rows_shifted": ("dense", "sparse", "gate"),          # (cases whose last row tile holds at least two rows)
    "tanh_gelu": ("gate",),
    "p_not_fp16": (),                                               # must PASS: the bound allows for the rounding, it does not demand it
}


def planted_units(p):
    """the two hidden units (same chunk, same k-step) a planted W2 error touches: the pair that feeds output channel 0 first"""
    u = sparse_w2_units(0)[0] if p["case"]["kind"] != "dense" else 5
    return u, u ^ 4          # bit 2: the same chunk and k-step, another lane group (and another output channel in the sparse layouts)


def emulate(case_id, planted=None):
    """the output the kernel's arithmetic gives in fp32 on the CPU: (out, mirror | None) in the case's output dtypes"""
    p = problem(case_id)
    f = FORMS[p["case"]["form"]]
    M = p["case"]["M"]
    w1, b1, w2 = p["w1"].float(), p["b1"].clone(), p["w2"].float().clone()
    if planted == "b1_of_next_chunk":          # chunk c takes the bias of chunk c + 1 (both halves)
        b1 = torch.cat([torch.roll(b1[:H], -HC), torch.roll(b1[H:], -HC)])
    y = p["x"].float() @ w1.t() + b1
    h, g = y[:, :H].clone(), y[:, H:].clone()
    if planted == "swap_hidden_gate_fragment":          # the 16 units of one MFMA fragment: unit planted_units()[0]'s
        u0 = planted_units(p)[0] & ~15
        h[:, u0:u0 + 16], g[:, u0:u0 + 16] = y[:, H + u0:H + u0 + 16], y[:, u0:u0 + 16]
    P = h * gelu_erf_f_emul(g, "tanh" if planted == "tanh_gelu" else "erf")
    if planted != "p_not_fp16":
        P = P.half().float()
    ua, ub = planted_units(p)
    if planted == "swap_w2_units":
        w2[:, [ua, ub]] = w2[:, [ub, ua]]
    if planted == "drop_unit":
        P[:, ua] = 0.0
    z = P @ w2.t()
    if p["b2"] is not None:
        z = z + p["b2"]
    if p["res"] is not None:
        z = z + p["res"].float()
    if p["mix"] is not None:
        al = 1.0 / (1.0 + torch.exp(-p["mix"].float()))
        z = al * p["blend_x"].float() + (1.0 - al) * z
    if planted == "last_tile_rows_shifted" and M - (M - 1) // 128 * 128 >= 2:
        r0 = (M - 1) // 128 * 128
        z[r0:M - 1] = z[r0 + 1:M].clone()
    return z.to(f["out"]), (z.half() if f["mirror"] else None)


def check(out, ref, bound):
    """worst |out - ref| / bound over the elements (fp64)"""
    return float(((out.double() - ref).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------------------------
# The packs, restated on the host
# ---------------------------------------------------------------------------------------------------------------------------
def geglu_pack_rows(N=2 * H):
    """packed row p of the GEGLU-interleaved W1 / b1 <- source row (csrc/elementwise.hip: geglu_src_row): blocks of 16 hidden rows and
    their 16 gate rows"""
    p = torch.arange(N)
    blk, wi = p >> 5, p & 31
    return torch.where(wi < 16, blk * 16 + wi, N // 2 + blk * 16 + wi - 16)


def w2_pack_index():
    """src[c'][n][col] of the W2 pack as the kernel's comment states it: the pack is [4][512][512]; inside chunk c of 128 hidden units
    (column block c >> 2, columns (c & 3) * 128 + kk), position kk = 32 kap + 8 q' + 2 q + i holds hidden unit
    32 q' + 16 (kap >> 1) + 4 q + 2 (kap & 1) + i of the chunk.  Returns the flat source index into W2 [512][2048] of every element of
    the flat pack."""
    n = torch.arange(D).view(1, D, 1)
    cb = torch.arange(4).view(4, 1, 1)
    col = torch.arange(512).view(1, 1, 512)
    c = cb * 4 + (col >> 7)
    kk = col & 127
    kap, qp, q, i = kk >> 5, (kk >> 3) & 3, (kk >> 1) & 3, kk & 1
    u = 32 * qp + 16 * (kap >> 1) + 4 * q + 2 * (kap & 1) + i
    return (n * H + c * HC + u).reshape(-1)


def pack_w1(w1):
    return w1[geglu_pack_rows()].contiguous()


def pack_w2(w2):
    return w2.reshape(-1)[w2_pack_index()].view(4, D, 512)


# ---------------------------------------------------------------------------------------------------------------------------
# Placement on the GPU: every operand inside a guarded allocation (tests/helpers.py: Guarded)
# ---------------------------------------------------------------------------------------------------------------------------
PAD_ROWS = 3


def _guard_rows(t, device, ld=None):
    """a [M][512] input inside NaN rows (and NaN pad columns when its stride is larger)"""
    from helpers import Guarded
    ld = ld or t.shape[1]
    return Guarded.inp(t, (PAD_ROWS, 0), (PAD_ROWS, ld - t.shape[1]), device)


def _guard_end(t, device):
    """a weight inside a flat NaN-guarded buffer that ENDS with it: the kernel's last piece of chunk 15 ends where the allocation ends"""
    from helpers import Guarded
    return Guarded.inp(t.reshape(-1), (64,), (0,), device)


def place(case_id, device, ops, outputs=1):
    """the case on the GPU: dict(x, w1, b1, w2p: Guarded inputs; res, blend_x: Guarded | None; outs: [ (out, mirror | None) Guarded ] *
    outputs; descs: one ctrl_ffn_desc per output set)"""
    from helpers import Guarded
    p = problem(case_id)
    c = p["case"]
    f, M = FORMS[c["form"]], c["M"]
    ld, ldres, ld16 = STRIDES[c["stride"]]
    q = dict(case=c)
    q["x"] = _guard_rows(p["x"], device)
    q["w1"] = _guard_end(pack_w1(p["w1"]), device)
    q["b1"] = _guard_end(p["b1"][geglu_pack_rows()], device)
    q["w2p"] = _guard_end(pack_w2(p["w2"]), device)
    q["b2"] = Guarded.inp(p["b2"], (4,), (4,), device) if p["b2"] is not None else None
    q["res"] = _guard_rows(p["res"], device, ldres) if p["res"] is not None else None
    q["blend_x"] = _guard_rows(p["blend_x"], device, ldres) if p["blend_x"] is not None else None
    q["mix"] = p["mix"].to(device) if p["mix"] is not None else None
    q["outs"], q["descs"] = [], []
    for _ in range(outputs):
        out = Guarded.out((M + 2 * PAD_ROWS, ld), (slice(PAD_ROWS, PAD_ROWS + M), slice(0, D)), f["out"], device)
        mir = Guarded.out((M + 2 * PAD_ROWS, ld16), (slice(PAD_ROWS, PAD_ROWS + M), slice(0, D)), torch.float16, device) if f["mirror"] else None
        q["outs"].append((out, mir))
        q["descs"].append(ops.ffn_desc(q["x"].view, q["w1"].view, q["b1"].view, q["w2p"].view, out.view,
                                       b2=q["b2"].view if q["b2"] is not None else None, res=q["res"].view if q["res"] is not None else None,
                                       out16=mir.view if mir is not None else None, ld=ld, ldres=ldres, ld16=ld16,
                                       blend_mix=q["mix"], blend_x=q["blend_x"].view if q["blend_x"] is not None else None, ld_blend=ldres))
    return q


def guards(q):
    return [g for g in (q["x"], q["w1"], q["b1"], q["w2p"], q["b2"], q["res"], q["blend_x"]) if g is not None] + \
           [g for pair in q["outs"] for g in pair if g is not None]
