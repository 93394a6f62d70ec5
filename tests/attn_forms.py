"""The pure-data part of tests/test_gpu_attn_forms.py: the table of attention kernel forms (FORMS), their edge cases, the construction
of a case's operands inside poisoned surroundings, the fp64 reference with its element-wise bound (helpers.attn_reference), and a plain
fp32 / fp16 emulation of the kernels' arithmetic that the host self-test (tests/test_attn_check_host.py) holds against the same bound."""
import contextlib
import functools
import math
import types

import torch

from helpers import Guarded, attn_reference

F16 = torch.float16
LOG2E = 1.4426950408889634
AO_NEGM, AO_SGB, AO_PRIO, AO_DEFER, AO_MINI, AO_DEFER8, AO_VPRIO = 1, 2, 4, 8, 16, 32, 64      # csrc/attention_d64.hip


def classic(D, NW, BATCH, FOLD):
    return "flash_attn_kernel<%d, %d, %s, %s>" % (D, NW, "true" if BATCH else "false", "true" if FOLD else "false")


def d64(QB, NW, OPT, NSTAGE=3):
    return "flash_attn_d64_kernel<%d, %d, %d, %d>" % (QB, NW, OPT, NSTAGE)


def d64p(OPT):
    return "flash_attn_d64p_kernel<%d>" % OPT


# op_flash_attn_d64: variant -> (symbol, queries per workgroup, ring depth)
D64_VARIANTS = {
    1: (d64(1, 8, 0), 256, 3),
    2: (d64(1, 8, AO_DEFER), 256, 3),
    3: (d64(1, 8, AO_DEFER8), 256, 3),
    4: (d64(1, 8, AO_DEFER | AO_PRIO), 256, 3),
    5: (d64(1, 8, AO_DEFER, 2), 256, 2),
    6: (d64(1, 4, AO_DEFER, 2), 128, 2),
    7: (d64(2, 4, AO_DEFER), 256, 3),
    8: (d64(2, 4, AO_DEFER | AO_PRIO), 256, 3),
    9: (d64p(AO_DEFER), 256, 3),
    10: (d64p(AO_MINI | AO_DEFER), 256, 3),
    11: (d64(1, 8, AO_MINI | AO_NEGM | AO_DEFER), 256, 3),
    12: (d64(1, 8, AO_DEFER, 4), 256, 4),
    13: (d64(2, 8, AO_DEFER), 512, 3),
    14: (d64(1, 8, AO_DEFER | AO_VPRIO), 256, 3),
}
DEFAULT_VARIANT = 2


class Case(dict):
    __getattr__ = dict.get


def C(name, **kw):
    kw.setdefault("B", 2)
    kw.setdefault("heads", 3)
    kw.setdefault("kind", "spike")
    return Case(name=name, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------------
LQ4 = (1, 31, 33, 128, 129, 200)                                    # 4-wave forms: 128 queries per workgroup, 32 per wave
LK4 = (1, 7, 8, 9, 63, 64, 65, 77, 128, 129, 192, 256, 261)         # 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5 tiles against the 3-deep ring; every
#                                                                     Lk % 8 class of the chunk straddling Lk; a last tile with 1 / 63 live keys
LQ8 = 2085                                                          # 8 * 256 + 37: one full wave, one wave of 5 queries, six waves past Lq
LK8 = (64, 77, 129, 257)
LK64 = (128, 192, 256, 320, 384, 448)                               # 2..7 tiles: every remainder of the rings of depth 2, 3, 4; the short
#                                                                     prologue of depth 4; the three epilogue slots of the pipelined kernel

FORMS = []


def form(sym, how, cases):
    FORMS.append((sym, how, cases))


def _four_wave(D, fold, tag, **kw):
    f = dict(D=D, fold=fold, **kw)
    cs = [C("%s Lq200 Lk%d" % (tag, lk), Lq=200, Lk=lk, **f) for lk in LK4]
    cs += [C("%s Lq%d Lk77" % (tag, lq), Lq=lq, Lk=77, **f) for lq in LQ4 if lq != 200]
    cs += [C("%s negative offset Lq129 Lk261" % tag, Lq=129, Lk=261, kind="neg", **f),
           C("%s negative offset Lq33 Lk65" % tag, Lq=33, Lk=65, kind="neg", **f),
           C("%s kvB1 Lq200 Lk77" % tag, Lq=200, Lk=77, kvB=1, **f),
           C("%s work map 10 pairs Lq129 Lk77" % tag, Lq=129, Lk=77, B=2, heads=5, **f)]
    return cs


for _D in (40, 80, 160, 64):
    for _fold in (False, True):
        _tag = "D%d %s" % (_D, "folded" if _fold else "plain")
        form(classic(_D, 4, True, _fold), "head dim %d%s%s" % (_D, ", k_prescaled" if _fold else "", ", Lq < 2048" if _D == 64 else ""),
             _four_wave(_D, _fold, _tag))

# the 4-wave form of head dim 64 at a long sequence: the CTRL_ATTN_NW4 policy entry (Lk = 77: no variant of attention_d64.hip applies)
for _fold in (False, True):
    form(classic(64, 4, True, _fold), "head dim 64, Lq >= 2048, CTRL_ATTN_NW4%s" % (", k_prescaled" if _fold else ""),
         [C("D64 %s NW4 Lq%d Lk77" % ("folded" if _fold else "plain", LQ8), D=64, fold=_fold, Lq=LQ8, Lk=77, heads=5, nw4=True)])

_w8 = dict(D=64, Lq=LQ8, B=2, heads=5)
form(classic(64, 8, False, False), "head dim 64, Lq >= 2048, K not pre-scaled",
     [C("D64 plain 8-wave Lk%d" % lk, Lk=lk, fold=False, **_w8) for lk in LK8]
     + [C("D64 plain 8-wave negative offset Lk77", Lk=77, fold=False, kind="neg", **_w8),
        C("D64 plain 8-wave kvB1 Lk129", Lk=129, fold=False, kvB=1, **_w8)])
form(classic(64, 8, False, True), "head dim 64, Lq >= 2048, k_prescaled and (Lk % 64 != 0 or Lk < 128 or kvB == 1 or variant 0)",
     [C("D64 folded 8-wave Lk%d" % lk, Lk=lk, fold=True, **_w8) for lk in LK8]
     + [C("D64 folded 8-wave variant0 Lk%d" % lk, Lk=lk, fold=True, variant=0, **_w8) for lk in (128, 192)]
     + [C("D64 folded 8-wave negative offset Lk77", Lk=77, fold=True, kind="neg", **_w8),
        C("D64 folded 8-wave kvB1 Lk128", Lk=128, fold=True, kvB=1, **_w8)])

for _v, (_sym, _qwg, _ns) in D64_VARIANTS.items():
    form(_sym, "head dim 64, k_prescaled, Lq >= 2048, Lk %% 64 == 0, Lk >= 128, kvB == B, set_attn_variant(%d)%s" % (
        _v, " (the default)" if _v == DEFAULT_VARIANT else ""),
         [C("d64 v%d Lk%d" % (_v, lk), Lk=lk, fold=True, variant=_v, **_w8) for lk in LK64]
         + [C("d64 v%d negative offset Lk320" % _v, Lk=320, fold=True, variant=_v, kind="neg", **_w8)])

ALL = [(sym, how, c) for sym, how, cs in FORMS for c in cs]

# temporal attention: F x (clips, pixels, heads); items = clips * pixels * heads, four per workgroup (1, 3, 5: dead waves)
TEMPORAL_F = (1, 2, 15, 16, 17, 31, 32)
TEMPORAL_ITEMS = ((1, 1, 1), (1, 3, 1), (1, 1, 5), (2, 12, 5))


# ------------------------------------------------------------------------------------------------------------------------------------
# operands, reference, bound
# ------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(shape, g, scale=1.0, shift=0.0):
    """fp16-representable fp32 values"""
    return (torch.randn(*shape, generator=g) * scale + shift).half().float()


def _heads(t, heads):           # [b][L][heads*D] -> [b][heads][L][D]
    b, L, Cc = t.shape
    return t.reshape(b, L, heads, Cc // heads).transpose(1, 2)


@functools.lru_cache(maxsize=24)
def _host_problem(D, fold, B, heads, Lq, Lk, kvB, kind, seed):
    """the fp16 operands of one problem (as fp32 CPU tensors) with the fp64 reference and bound; shared by every form that runs the
    shape (the 14 variants of attention_d64.hip see the same six problems) and never modified"""
    Cc = heads * D
    c = LOG2E / math.sqrt(D)
    g = _gen(7919 * seed + 31 * Lq + Lk + D)
    if kind == "neg":
        # a shared component +a on every element of Q and -a on K: every true score sits near -a^2 * D * c = -24 in the exp2 domain, so a
        # phantom key of score 0 (the zero-page K row a wrong mask admits) takes nearly all the weight, and the first tile is all-negative
        a = math.sqrt(24.0 / (c * D))
        q, k = _h((B, Lq, Cc), g, shift=a), _h((kvB, Lk, Cc), g, shift=-a)
    else:
        q, k = _h((B, Lq, Cc), g), _h((kvB, Lk, Cc), g)
        # one key of the LAST tile spiked against one query (the rescale path), one key of the FIRST tile against another
        jl = (Lk - 1) // 64 * 64 + ((Lk - 1) % 64) // 2
        k[0, jl] = q[0, min(5, Lq - 1)] * 4.0
        k[kvB - 1, min(3, Lk - 1)] = q[B - 1, min(100, Lq - 1)] * 6.0
        k = k.half().float()                                 # (6 q needs a mantissa bit more than q has: round, so both sides see one K)
    v = _h((kvB, Lk, Cc), g)
    if fold:
        kdev = (k * c).half().float()           # what the producing GEMM hands over: k * scale * log2(e), rounded ONCE
        ref, bound = attn_reference(_heads(q, heads), _heads(kdev, heads), _heads(v, heads), 1.0)
    else:
        kdev = k
        ref, bound = attn_reference(_heads(q, heads), _heads(kdev, heads), _heads(v, heads), c)
    Lkpad = (Lk + 63) // 64 * 64
    r8 = (Lk + 7) // 8 * 8
    vt = torch.full((kvB, Cc, Lkpad), float("nan"))
    vt[:, :, :r8] = 60000.0                       # the contract asks for FINITE pad columns [Lk, roundup8(Lk)), not for zeros
    vt[:, 1::2, :r8] = -60000.0
    vt[:, :, :Lk] = v.permute(0, 2, 1)
    fin = lambda t: t.transpose(1, 2).reshape(B * Lq, Cc).contiguous()
    return types.SimpleNamespace(q=q, k=kdev, v=v, vt=vt, ref=fin(ref), bound=fin(bound), Lkpad=Lkpad, c=1.0 if fold else c)


def host_problem(c, seed=0):
    return _host_problem(c.D, bool(c.fold), c.B, c.heads, c.Lq, c.Lk, c.kvB or c.B, c.kind, seed)


def make_problem(ops, device, c, seed=0):
    """the operands of case `c` inside poisoned surroundings on `device`, with the descriptor arguments over them:
    Q and K as thirds of [rows + guard][3 C + 8] rows (NaN pad columns and guard rows), V^T followed by NaN rows, O at ld = C + 12 (ld % 4,
    its first row 8-byte but not 16-byte aligned) between guard rows"""
    H = host_problem(c, seed)
    B, heads, D, Lq, Lk = c.B, c.heads, c.D, c.Lq, c.Lk
    kvB = c.kvB or B
    Cc = heads * D
    ld = 3 * Cc + 8
    P = types.SimpleNamespace(H=H, ref=H.ref, bound=H.bound)
    P.Q = Guarded.inp(H.q.reshape(B * Lq, Cc).half(), (3, 0), (5, ld - Cc), device)
    P.K = Guarded.inp(H.k.reshape(kvB * Lk, Cc).half(), (3, Cc), (5, ld - 2 * Cc), device)
    P.Vt = Guarded.inp(H.vt.reshape(kvB * Cc, H.Lkpad).half(), (0, 0), (4, 0), device)
    P.O = Guarded.out((1 + B * Lq + 6, Cc + 12), (slice(1, 1 + B * Lq), slice(0, Cc)), F16, device)
    assert P.O.view.data_ptr() % 16 == 8
    P.args = (P.Q.view, ld, P.K.view, ld, P.Vt.view, H.Lkpad, B, heads, D, Lq, Lk)
    P.kw = dict(kvB=kvB, k_prescaled=bool(c.fold), out=P.O.view, ldo=Cc + 12)
    return P


@contextlib.contextmanager
def dispatch(ops, c):
    """brings the dispatcher to the case's form (variant, CTRL_ATTN_NW4); both restored on the way out"""
    prev = None
    try:
        if c.nw4:
            prev = ops.set_policy("CTRL_ATTN_NW4", "1")
        if c.variant is not None:
            ops.set_attn_variant(c.variant)
        yield
    finally:
        if c.variant is not None:
            ops.set_attn_variant(-1)
        if c.nw4:
            ops.set_policy("CTRL_ATTN_NW4", prev)


def temporal_problem(Bc, Fr, HW, heads, seed=0):
    """q | k | v rows [(b f) p][3 C] (fp16-representable fp32) with the fp64 reference and bound in the same row order"""
    Cc = heads * 64
    g = _gen(104729 * seed + 97 * Fr + Bc * HW * heads)
    qkv = _h((Bc, Fr, HW, 3, heads, 64), g)
    qkv[0, Fr - 1, 0, 1] = qkv[0, 0, 0, 0] * 4.0           # the last key frame spiked against the first query frame of one pixel
    seq = lambda i: qkv[:, :, :, i].permute(0, 2, 3, 1, 4)   # [b][p][h][f][64]
    ref, bound = attn_reference(seq(0), seq(1), seq(2), LOG2E / 8.0, p_fp16=False)
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(Bc * Fr * HW, Cc).contiguous()
    return qkv.reshape(Bc * Fr * HW, 3 * Cc), back(ref), back(bound)


# ------------------------------------------------------------------------------------------------------------------------------------
# a plain emulation of the kernels' arithmetic (fp32 scores and sums, P rounded to fp16 for P . V, a reference point that moves only when
# a score passes it by more than `thr`, fp16 result) -- what the bound is held against where there is no GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, c, fold, thr=4.0, phantom=False):
    """q [N][Lq][D], k, v [N][Lk][D] fp16-representable; 64-key tiles.  phantom: the last tile admits one key past Lk whose K row is the
    zero page (score 0) -- the off-by-one mask this suite has to catch."""
    q, k, v = q.float(), k.float(), v.float()
    N, Lq, D = q.shape
    Lk = k.shape[1]
    if phantom:
        k = torch.cat([k, torch.zeros(k.shape[0], 1, D)], 1)
        v = torch.cat([v, torch.zeros(v.shape[0], 1, D)], 1)
    cf = torch.tensor(1.0 if fold else c, dtype=torch.float32)
    m = torch.zeros(N, Lq, 1) if fold else torch.full((N, Lq, 1), -1e30)
    l = torch.zeros(N, Lq, 1)
    o = torch.zeros(N, Lq, D)
    for t0 in range(0, k.shape[1], 64):
        kt, vt = k[:, t0:t0 + 64], v[:, t0:t0 + 64]
        s = q @ kt.transpose(1, 2)
        if fold:
            s = s - m                                        # (the kernel starts the accumulator at -m)
            mx = s.max(-1, keepdim=True).values
            d = mx if t0 == 0 else torch.where(mx > thr, mx.clamp_min(0.0), torch.zeros_like(mx))
            alpha = torch.ones_like(d) if t0 == 0 else torch.exp2(-d)
            m = m + d
            s = s - d
        else:
            m_new = torch.maximum(m, s.max(-1, keepdim=True).values * cf)
            alpha = torch.exp2(m - m_new)
            m = m_new
            s = s * cf - m
        p = torch.exp2(s)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.half().float() @ vt
    return (o * (1.0 / l)).half()
