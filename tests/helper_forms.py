"""The layout, packing and small helper kernels (csrc/elementwise.hip, and unet_conv_out / i2v_frames of csrc/unet.hip, vae_conv_in /
vae_row_softmax of csrc/vae.hip) at their tile, chunk, wrap and grid-stride edges: case tables, problem builders seeded by case id, fp64
references with element-wise bounds or exact restatements, fp32 emulations in the kernels' own association and the planted errors the
checks have to reject.  Pure data: imports no GPU code.

    GPU tests: tests/test_gpu_helper_forms.py        host self-test (no GPU): tests/test_helper_check_host.py

u = 2^-24 (half an fp32 ulp, relative); quantum(ref, dt) one quantum of the output type at |ref| (0 for fp32 where the fp32 value itself
is what the bound speaks of, else as tower_forms.quantum).

Exact families.  A kernel that moves a value, or applies ONE fp32 operation and ONE rounding to the output type, is restated in torch
    with the same operations and compared bit for bit: the transposes (one product x * scale, one conversion), add_rowvec (one fp32 add, one
    conversion), i2v_frames (a conversion to fp32), every packer (a conversion to fp16 / fp32; the phase pack adds at most four fp32
    values in (ky, kx) order -- an addition cannot be contracted).  The grid-stride second trips of avgpool, blend and merge run over
    small dyadic values, for which every product and sum is exact in fp32 whatever the compiler contracts.
avgpool.  s = the fp32 sum of n = ky kx values in window order (n - 1 roundings), times inv = fp32(1 / n) (the constant's rounding and
    the product's): (n + 1) u mean|x| + one quantum of the output type (the store).
sincos.  freq = expf(-c k / half) with c = fp32(ln 1e4), arg = t freq, out = cos | sin (arg).  With x = ln(1e4) k / half the exponent:
    the constant, the product c k and the quotient each cost u relative to x, i.e. 3 u x relative to freq; expf costs its own ulps; the
    product t freq one u: |d arg| <= |arg| (A x + B) u, and |d cos|, |d sin| <= |d arg|; cosf / sinf add C u (|out| <= 1).
    C is calibrated alone on the columns k = 0, where x = 0, freq = 1 and arg = t are exact so that only cosf / sinf err (bound C u);
    then A = B = SC_K on the whole table (the data cannot tell the two apart: one power of two for both).
linear_small.  out = act_out(act_in(x) W^T + b), x fp32, W fp16, fp32 accumulation: helpers.igemm_bound's (K + 8) u mag in any order, mag =
    |act_in(x)| |W|^T + |b|; in_silu: every operand carries tower_forms' e_quick at k = 1 (x sigmoid(x) = x rcp(1 + __expf(-x))), summed
    with |W|; out_silu: slope 1.1 on the pre-activation's error + e_quick at |v| + dv.  No output rounding: the fp32 value is the result.
blend.  alpha = 1 / (1 + __expf(-mix)), y = alpha a + (1 - alpha) b.  e = exp(-mix) carries 2 u |mix| (log2 e and the product in front of
    v_exp_f32) + the exponential's ulps, enters alpha with weight (1 - alpha); 1 + e, the division: d alpha <= alpha ((1 - alpha) (2 |mix|
    + 2) + 2) u BL_K; 1 - alpha rounds once more; two products and one sum: 3 u (alpha |a| + (1 - alpha) |b|);
    bound = d alpha (|a| + |b|) + u |b| + 3 u (alpha |a| + (1 - alpha) |b|) + one quantum of the output.  BL_K calibrated (an expf figure).
merge.  out = sum_k w[widx[k]] x_k in expert order: K products and K sums, (K + 1) u sum |w| |x| in any contraction + one output quantum.
router.  softmax over the logits, a masked one lowered by 1e6 (so that its exponential is exactly 0 beside a live one).  d_i = l_i - max:
    bound = RT_K u ref (1 + |d_i| + max_j |d_j| + E) + 2^-126 (a flushed denormal: exp(-100) is one), the maximum over the experts that are not exactly 0.  RT_K calibrated.
unet_conv_out / vae_conv_in.  fp32 fma chains over 9 C (27) products in any order + the lane exchange and the bias:
    (9 C + 8) u mag + one output quantum; (27 + 2) u mag, mag = |x| * |w| + |b|.
vae_row_softmax.  P = fp16(expf(s - m) / z): one fp16 quantum + SM_K u ref (1 + |s - m|).  SM_K calibrated.  The pad columns are +0.
    Kinds: plain (sigma 6); constant (z = L exactly, every entry fp16(1 / L) bit for bit); spike_first / spike_last (one entry 80 above
    the rest: 1 beside exact zeros, bit for bit); step (the entries from 256 on 120 higher).  A softmax does not depend on the point it is
    shifted by, so a maximum taken over too few entries shows only where exp overflows: 80 above does not reach fp32's 88.7, the step does.

Calibrated constants (the smallest power of two for which the fp32 CPU emulation, in the kernel's association, stays at or below 0.5 of
the bound on this table; the factor 2 is the margin for the device's expf, sinf, cosf and rcp differing from the host's, which nobody has
measured here).  Printed by tests/test_helper_check_host.py::test_emulations_stay_within_their_bounds:
    SC_C = 2^1     share 0.25 on the k = 0 columns; 2^0 gives 0.51
    SC_K = 2^2     share 0.30 on the whole table;   2^1 gives 0.54
    BL_K = 2^-1    share 0.43 (of what the bound holds beyond the output quantum, the half quantum of a correct store taken off the
                   error); 2^-2 gives 0.52
    RT_K = 2^0     share 0.42;                      2^-1 gives 0.83
    SM_K = 2^3     share 0.37 (the fp32 value before the fp16 store against the SM_K term alone: the store's half quantum hides every
                   fp32 effect); 2^2 gives 0.74
"""
import functools
import math
import zlib

import torch

import helpers
import norm_forms as NF
import tower_forms as TF

U = 2.0 ** -24
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
DT_NAME = TF.DT_NAME
POISON = helpers._POISON

# restated from the .hip files
TILE_C, TILE_P, THREADS = 32, 64, 256          # nchw_to_nhwc_kernel / nhwc_to_nchw_kernel: 32 c x 64 p per workgroup of 256
GRID_CAP = 8192                                # grid_for
TRIP = GRID_CAP * THREADS                      # work items of one grid-stride trip
LS_MT, LS_COLS, LS_KTRIP = 8, 4, 512           # linear_small_kernel<8>: 8 rows, four columns (one per wave), 64 lanes x 8 k per trip
CO_LANES, CO_PIX = 4, 64                       # unet_conv_out_kernel: four lanes per pixel, 64 pixels per workgroup
CI_GROUP = 16                                  # vae_conv_in_kernel: 16 output channels per thread
SM_THREADS = 256                               # vae_row_softmax_kernel
FP16_MAX = 65504.0

SC_C, SC_K, BL_K, RT_K, SM_K = 2.0 ** 1, 2.0 ** 2, 2.0 ** -1, 2.0 ** 0, 2.0 ** 3


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def pick(table, **want):
    """the first case of a table with these attributes"""
    return next(c for c in table if all(c[k] == v for k, v in want.items()))


Case = TF.Case
quantum = TF.quantum


def out_quantum(ref, dt):
    return quantum(ref, dt) if dt != F32 else torch.zeros_like(ref)


def check(out, ref, bound):
    """worst |out - ref| / bound (fp64); inf when an output is not finite"""
    return TF.check(out, ref, bound)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(helpers._bits(a), helpers._bits(b)))


def plus_one_ulp16(t, index=0):
    """planted: one fp16 ulp added to one element of an exact fp16 result"""
    t = t.clone()
    flat = t.view(-1)
    b = flat[index:index + 1].view(torch.int16)
    b += 1
    return t


def odd_values(shape, dt, g, scale=3.0):
    """values that are not fp16-representable where the type allows it"""
    return (torch.randn(shape, generator=g) * scale).to(dt)


# ---------------------------------------------------------------------------------------------------------------------------
# transposes
# ---------------------------------------------------------------------------------------------------------------------------
TR_NS, TR_CS, TR_HWS, TR_SCALES = (1, 3), (1, 31, 32, 33, 70), (1, 63, 64, 65, 130), (1.0, 0.5, 0.18215)
TRANSPOSE = []
for _i, (_N, _C, _HW) in enumerate((n, c, p) for n in TR_NS for c in TR_CS for p in TR_HWS):
    _dt, _sc = DTYPES[_i % 3], TR_SCALES[(_i // 3) % 3]
    TRANSPOSE.append(Case(id="tr-N%d-C%d-HW%d-%s-s%g" % (_N, _C, _HW, DT_NAME[_dt], _sc), N=_N, C=_C, HW=_HW, dt=_dt, scale=_sc, map=None, ndst=_N))
for _j, (_C, _HW) in enumerate(((33, 65), (70, 130), (1, 1))):
    TRANSPOSE.append(Case(id="tr-perm-C%d-HW%d-%s" % (_C, _HW, DT_NAME[DTYPES[_j]]), N=3, C=_C, HW=_HW, dt=DTYPES[_j], scale=TR_SCALES[_j],
                          map=(2, 0, 1), ndst=3))
    TRANSPOSE.append(Case(id="tr-scatter-C%d-HW%d-%s" % (_C, _HW, DT_NAME[DTYPES[_j]]), N=3, C=_C, HW=_HW, dt=DTYPES[_j], scale=TR_SCALES[2 - _j],
                          map=(4, 0, 2), ndst=5))
# the special values through the bf16 store (f32_to_bf16 rounds a NaN as a number: csrc/common.h)
TRANSPOSE.append(Case(id="tr-special-bf16", N=1, C=8, HW=3, dt=BF16, scale=1.0, map=None, ndst=1, special=True))
TR_BY_ID = {c.id: c for c in TRANSPOSE}


def to_nhwc_problem(c):
    """x [N][C][HW] of c.dt (the source type), want fp16 [N][HW][C]"""
    x = odd_values((c.N, c.C, c.HW), c.dt, _gen("to_nhwc", c.id))
    return x, x.float().half().transpose(1, 2).contiguous()


def to_nchw_problem(c, planted=None):
    """x fp16 [N][HW][C]; want [ndst][C][HW] of c.dt, images nothing maps to left at poison.
    planted: last_c_row | last_p_col (the last channel of the last channel tile / pixel of the last pixel tile left unwritten), map_ignored"""
    x = odd_values((c.N, c.HW, c.C), F16, _gen("to_nchw", c.id))
    if c.special:
        x.view(-1)[:4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 65504.0], dtype=F16)
    y = (x.float() * torch.tensor(c.scale, dtype=F32)).to(c.dt).transpose(1, 2).contiguous()
    if planted == "last_c_row":
        y[:, c.C - 1, :] = POISON[c.dt]
    if planted == "last_p_col":
        y[:, :, c.HW - 1] = POISON[c.dt]
    want = torch.full((c.ndst, c.C, c.HW), POISON[c.dt], dtype=c.dt)
    for n in range(c.N):
        want[c.map[n] if (c.map and planted != "map_ignored") else n] = y[n]
    return x, want


# ---------------------------------------------------------------------------------------------------------------------------
# avgpool
# ---------------------------------------------------------------------------------------------------------------------------
AP_SHAPES = ((4, 4, 4, 4), (6, 4, 2, 2), (8, 8, 1, 1), (2, 6, 1, 3))
AP_REFUSED = (6, 4, 4, 4)
AVGPOOL = [Case(id="ap-%dx%d-%dx%d-NC%d-%s" % (s + (nc, DT_NAME[dt])), shape=s, NC=nc, dt=dt) for s in AP_SHAPES for nc in (1, 5) for dt in DTYPES]
AP_SECOND = Case(id="ap-second-trip-2050x2048-1025x2048-f16", shape=(2050, 2048, 1025, 2048), NC=1, dt=F16)          # 1025 * 2048 outputs > TRIP


def avgpool_problem(c):
    """x [NC][Hin][Win], ref, bound fp64 [NC][Hout][Wout]"""
    Hin, Win, Hout, Wout = c.shape
    x = odd_values((c.NC, Hin, Win), c.dt, _gen("ap", c.id))
    ky, kx = Hin // Hout, Win // Wout
    w = x.double().reshape(c.NC, Hout, ky, Wout, kx)
    ref = w.mean((2, 4))
    bound = (ky * kx + 1) * U * w.abs().mean((2, 4)) + quantum(ref, c.dt)
    return x, ref, bound


def avgpool_emulate(c):
    Hin, Win, Hout, Wout = c.shape
    x, _, _ = avgpool_problem(c)
    ky, kx = Hin // Hout, Win // Wout
    w = x.float().reshape(c.NC, Hout, ky, Wout, kx)
    s = torch.zeros(c.NC, Hout, Wout)
    for a in range(ky):
        for b in range(kx):
            s = s + w[:, :, a, :, b]
    return (s * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(ky * kx), dtype=F32))).to(c.dt)


def avgpool_second_trip():
    """dyadic fp16 data (multiples of 1/4 in [-8, 8)): the sum of two and its half are exact; want fp16, bit for bit"""
    Hin, Win, Hout, Wout = AP_SECOND.shape
    x = (torch.randint(-32, 32, (1, Hin, Win), generator=_gen("ap2"), dtype=torch.int32).float() / 4.0).half()
    want = ((x[:, 0::2].float() + x[:, 1::2].float()) * 0.5).half()
    return x, want


# ---------------------------------------------------------------------------------------------------------------------------
# sincos
# ---------------------------------------------------------------------------------------------------------------------------
SC_TS = (0.0, 1.0, 250.5, 999.0)
SINCOS = [Case(id="sc-N%d-tc%d-dim%d" % (N, tc, dim), N=N, t_count=tc, dim=dim) for N in (1, 3) for tc in sorted({1, N}) for dim in (2, 6, 320)]
LN1E4 = 9.210340371976184


def sincos_t(c, which):
    """the timesteps of a case: `which` walks SC_TS so that every t meets every shape"""
    return torch.tensor([SC_TS[(which + i) % 4] for i in range(c.t_count)], dtype=F32)


def sincos_problem(c, which):
    """t, ref, bound [N][dim], exact_arg mask (k == 0)"""
    t = sincos_t(c, which)
    half = c.dim // 2
    k = torch.arange(half, dtype=torch.float64)
    x = LN1E4 * k / half
    arg = (t.double().expand(c.N) if c.t_count == 1 else t.double())[:, None] * torch.exp(-x)[None, :]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    darg = arg.abs() * (SC_K * x[None, :] + SC_K) * U
    darg = torch.where((k == 0)[None, :], torch.zeros_like(darg), darg)          # x = 0: freq = 1 and arg = t are exact
    bound = torch.cat([darg, darg], 1) + SC_C * U
    return t, ref, bound, torch.cat([k == 0, k == 0])[None, :].expand(c.N, c.dim)


def sincos_emulate(c, which):
    t = sincos_t(c, which)
    half = c.dim // 2
    k = torch.arange(half, dtype=F32)
    freq = torch.exp(torch.tensor(-LN1E4, dtype=F32) * k / torch.tensor(float(half), dtype=F32))
    arg = (t.expand(c.N) if c.t_count == 1 else t)[:, None] * freq[None, :]
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# linear_small
# ---------------------------------------------------------------------------------------------------------------------------
LS_MS, LS_NS, LS_KS = (1, 7, 8, 9, 17), (1, 3, 4, 5, 333), (8, 504, 512, 520, 1288)
LINEAR = []
for _i, (_M, _N, _K) in enumerate((m, n, k) for m in LS_MS for n in LS_NS for k in LS_KS):
    _f = (_i + _i // 5 + _i // 25) % 8
    LINEAR.append(Case(id="ls-M%d-N%d-K%d%s%s%s" % (_M, _N, _K, "-bias" if _f & 1 else "", "-in" if _f & 2 else "", "-out" if _f & 4 else ""),
                       M=_M, N=_N, K=_K, bias=bool(_f & 1), in_silu=bool(_f & 2), out_silu=bool(_f & 4)))
LS_BY_ID = {c.id: c for c in LINEAR}
LS_MAXM = max(LS_MS)


@functools.lru_cache(maxsize=None)
def linear_operands(N, K):
    """x [17][K] fp32, W [N][K] fp16, bias [N] fp32: a case of M rows takes the first M"""
    g = _gen("ls", N, K)
    return (torch.randn(LS_MAXM, K, generator=g) * 1.5, (torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K))).half(),
            torch.randn(N, generator=g))


def _equick(v_hi, v):
    """tower_forms' e_quick at k = 1"""
    s = torch.sigmoid(v)
    return v_hi * s * (4 * U + (1 - s) * (4 * U * v_hi + 2 * U)) + 2.0 ** -126


def linear_reference(c):
    x, W, b = linear_operands(c.N, c.K)
    x, W = x[:c.M].double(), W.double()
    a, ea = x, torch.zeros_like(x)
    if c.in_silu:
        a, ea = NF.silu64(x), _equick(x.abs(), x)
    v = a @ W.t()
    mag = a.abs() @ W.abs().t()
    dv = ea @ W.abs().t()
    if c.bias:
        v, mag = v + b.double(), mag + b.double().abs()
    dv = dv + (c.K + 8) * U * mag
    if not c.out_silu:
        return v, dv
    return NF.silu64(v), 1.1 * dv + _equick(v.abs() + dv, v)


def _silu32(x):
    return x * (1.0 / (1.0 + torch.exp(-x)))


def linear_emulate(c, planted=None):
    """lane l of a column's wave takes k = 8 l + 512 trip + j in order, then the butterfly; planted: drop_last_trip, drop_last_col_of_wg"""
    x, W, b = linear_operands(c.N, c.K)
    x, W = x[:c.M].float(), W.float()
    if c.in_silu:
        x = _silu32(x)
    trips = -(-c.K // LS_KTRIP)
    Kp = trips * LS_KTRIP
    xp = NF._pad(x, 1, Kp).reshape(c.M, 1, trips, 64, 8)
    wp = NF._pad(W, 1, Kp).reshape(1, c.N, trips, 64, 8)
    acc = torch.zeros(c.M, c.N, 64)
    for tr in range(trips - (1 if planted == "drop_last_trip" and trips > 1 else 0)):
        for j in range(8):
            acc = acc + xp[:, :, tr, :, j] * wp[:, :, tr, :, j]
    v = NF._xor_tree(acc, 64)
    if c.bias:
        v = v + b
    if c.out_silu:
        v = _silu32(v)
    if planted == "drop_last_col_of_wg" and c.N % LS_COLS:
        v = v.clone()
        v[:, c.N - 1] = POISON[F32]
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------------
BL_CHUNKS, BL_MIX = (1, 255, 257), (0.0, 0.3, -20.0, 20.0)
BLEND = []
for _i, (_a, _b, _y) in enumerate((a, b, y) for a in (F16, F32) for b in (F16, F32) for y in (F16, F32)):
    for _j, _ch in enumerate(BL_CHUNKS):
        for _m in BL_MIX:
            BLEND.append(Case(id="bl-%s-%s-%s-ch%d-mix%g" % (DT_NAME[_a], DT_NAME[_b], DT_NAME[_y], _ch, _m), xs=_a, xt=_b, y=_y, chunks=_ch, mix=_m))
BL_SECOND_CHUNKS = TRIP + 257


def blend_problem(c):
    g = _gen("bl", c.id)
    n = 8 * c.chunks
    a, b = odd_values((n,), c.xs, g), odd_values((n,), c.xt, g)
    m = float(torch.tensor(c.mix, dtype=F32))
    al = 1.0 / (1.0 + math.exp(-m))
    a64, b64 = a.double(), b.double()
    ref = al * a64 + (1.0 - al) * b64
    dal = al * ((1.0 - al) * (2.0 * abs(m) + 2.0) + 2.0) * U * BL_K
    bound = dal * (a64.abs() + b64.abs()) + U * b64.abs() + 3 * U * (al * a64.abs() + (1.0 - al) * b64.abs()) + out_quantum(ref, c.y) + 2.0 ** -149
    return a, b, ref, bound


def blend_emulate(c):
    a, b, _, _ = blend_problem(c)
    al = torch.tensor(1.0, dtype=F32) / (1.0 + torch.exp(-torch.tensor(c.mix, dtype=F32)))
    return (al * a.float() + (1.0 - al) * b.float()).to(c.y)


def blend_second_trip():
    """mix = 0: alpha = 0.5 exactly; dyadic fp16 data: y = (a + b) / 2 exactly"""
    n = 8 * BL_SECOND_CHUNKS
    g = _gen("bl2")
    a = (torch.randint(-32, 32, (n,), generator=g, dtype=torch.int32).float() / 4.0).half()
    b = (torch.randint(-32, 32, (n,), generator=g, dtype=torch.int32).float() / 4.0).half()
    return a, b, ((a.float() + b.float()) * 0.5).half()


# ---------------------------------------------------------------------------------------------------------------------------
# add_rowvec
# ---------------------------------------------------------------------------------------------------------------------------
ADDV = []
for _i, (_C, _r, _vm) in enumerate((c, r, v) for c in (8, 328) for r in (1, 5) for v in (1, 2, 3)):
    _M = (2 * _vm + 1) * _r - (_r // 2)            # 2 vmod + 1 images (no multiple of vmod), the last one partial when rows_per_img > 1
    _x, _y = ((F16, F16), (F32, F32), (F16, F32), (F32, F16))[_i % 4]
    ADDV.append(Case(id="av-C%d-r%d-vmod%d-M%d-%s-%s%s" % (_C, _r, _vm, _M, DT_NAME[_x], DT_NAME[_y], "-inplace" if _x == _y and _i % 8 < 4 else ""),
                     C=_C, rows_per_img=_r, vmod=_vm, M=_M, x=_x, y=_y, inplace=_x == _y and _i % 8 < 4))
AV_SECOND = Case(id="av-second-trip-C8-r7-vmod3", C=8, rows_per_img=7, vmod=3, M=TRIP + 300, x=F16, y=F16, inplace=False)


def addv_index(M, rows_per_img, vmod, planted=None):
    """planted vmod_off_by_one: the wrap at vmod + 1"""
    return (torch.arange(M) // rows_per_img) % (vmod + 1 if planted == "vmod_off_by_one" else vmod)


def addv_problem(c, planted=None):
    """x [M][C], v [vmod + 1][C] fp32 (one row more than the kernel may read), want [M][C] of c.y"""
    g = _gen("av", c.id)
    if c.M > 4096:
        x = (torch.randint(-512, 512, (c.M, c.C), generator=g, dtype=torch.int32).float() / 16.0).to(c.x)
    else:
        x = odd_values((c.M, c.C), c.x, g)
    v = torch.randn(c.vmod + 1, c.C, generator=g)
    return x, v, (x.float() + v[addv_index(c.M, c.rows_per_img, c.vmod, planted)]).to(c.y)


# ---------------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------------
MERGE = [Case(id="mg-K%d-n%d-%s" % (K, n, DT_NAME[dt]), K=K, n=n, dt=dt, E=K + 3) for K in (1, 3, 8) for n in (1, 255, 257) for dt in DTYPES]
MERGE.append(Case(id="mg-special-bf16", K=1, n=8, dt=BF16, E=2, special=True))
MG_SECOND_N = TRIP + 257


def merge_widx(c):
    """a non-identity selection of K out of E weights"""
    return [(2 * k + 1) % c.E if c.E % 2 else (k + 2) % c.E for k in range(c.K)] if not c.special else [1]


def merge_problem(c):
    """xs K tensors [n] of c.dt, w [E] fp32, widx, ref, bound"""
    g = _gen("mg", c.id)
    xs = [odd_values((c.n,), c.dt, g) for _ in range(c.K)]
    w = torch.softmax(torch.randn(c.E, generator=g), 0)
    widx = merge_widx(c)
    if c.special:          # weight 1: nan, +-inf and the largest finite fp32-rounded values pass through the cast
        w = torch.tensor([0.25, 1.0])
        xs[0][:4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38]).to(BF16)
    ref = sum(w[widx[k]].double() * xs[k].double() for k in range(c.K))
    mag = sum(w[widx[k]].double().abs() * xs[k].double().abs() for k in range(c.K))
    return xs, w, widx, ref, (c.K + 1) * U * mag + out_quantum(ref, c.dt) + 2.0 ** -149


def merge_emulate(c):
    xs, w, widx, _, _ = merge_problem(c)
    s = torch.zeros(c.n)
    for k in range(c.K):
        s = s + w[widx[k]] * xs[k].float()
    return s.to(c.dt)


# ---------------------------------------------------------------------------------------------------------------------------
# router
# ---------------------------------------------------------------------------------------------------------------------------
RT_ES, RT_RS = (1, 3, 16), (1, 64, 65)
RT_MASKS = ("none", "one", "all_but_one", "all")
ROUTER = [Case(id="rt-E%d-R%d-%s%s" % (E, R, m, "-equal" if eq else ""), E=E, R=R, mask=m, equal=eq)
          for E in RT_ES for R in RT_RS for m in RT_MASKS for eq in (False, True) if not (E == 1 and m in ("one", "all_but_one"))]


def router_mask(c):
    if c.mask == "none":
        return None
    if c.mask == "one":
        return [0 if e == c.E // 2 else 1 for e in range(c.E)]
    if c.mask == "all_but_one":
        return [1 if e == c.E - 1 else 0 for e in range(c.E)]
    return [0] * c.E


def router_problem(c):
    """wg [R][E] fp32 (None with equal weights), mask, ref, bound, dead (the experts that must be exactly 0).
    Row 0 holds logits of +-50; with every expert masked the rows are constant (the lowered logits round, and only equal ones give a
    reference of their own: the uniform distribution)."""
    g = _gen("rt", c.id)
    wg = torch.randn(c.R, c.E, generator=g) * 3.0
    wg[0] = torch.tensor([50.0 if e % 2 == 0 else -50.0 for e in range(c.E)])
    if c.mask == "all":
        wg = wg[:, :1].expand(c.R, c.E).contiguous()
    m = router_mask(c)
    lg = torch.zeros(c.R, c.E, dtype=torch.float64) if c.equal else wg.double()
    live = torch.tensor([1] * c.E if m is None else m, dtype=torch.bool)
    if c.mask == "all":
        live = torch.ones(c.E, dtype=torch.bool)          # every logit lowered alike
    lm = torch.where(live[None, :], lg, torch.full_like(lg, -float("inf")))
    ref = torch.softmax(lm, 1)
    d = torch.where(live[None, :], lm - lm.max(1, keepdim=True).values, torch.zeros_like(lm))
    bound = RT_K * U * ref * (1.0 + d.abs() + d.abs().max(1, keepdim=True).values + c.E) + 2.0 ** -126
    return (None if c.equal else wg), m, ref, bound, ~live


def router_emulate(c, planted=None):
    """planted mask_not_in_sum: the maximum sees the lowered logits, the sum the plain ones"""
    wg, m, _, _, _ = router_problem(c)
    v = torch.zeros(c.R, c.E) if wg is None else wg.clone()
    low = v.clone()
    if m is not None:
        low[:, [e for e in range(c.E) if m[e] == 0]] -= torch.tensor(1e6, dtype=F32)
    mx = low.max(1, keepdim=True).values
    ex = torch.exp((v if planted == "mask_not_in_sum" else low) - mx)
    s = torch.zeros(c.R)
    for e in range(c.E):
        s = s + ex[:, e]
    return ex / s[:, None]


# ---------------------------------------------------------------------------------------------------------------------------
# packers
# ---------------------------------------------------------------------------------------------------------------------------
PK_CONV = [Case(id="pk-conv-Co%d-Ci%d-t%d-%s" % (co, ci, t, DT_NAME[DTYPES[(co + ci + t) % 3]]), Cout=co, Cin=ci, taps=t, dt=DTYPES[(co + ci + t) % 3])
           for co in (1, 5) for ci in (1, 3, 8) for t in (1, 3, 9)]
PK_DIRECT = [Case(id="pk-direct-Co%d-Ci%d-%s" % (co, ci, DT_NAME[DTYPES[(co + ci) % 3]]), Cout=co, Cin=ci, taps=9, dt=DTYPES[(co + ci) % 3])
             for co in (1, 5) for ci in (1, 3, 8)]
PK_LINEAR = [Case(id="pk-lin-N%d-K%d-%s%s" % (N, K, DT_NAME[DTYPES[(N // 8 + K + g) % 3]], "-geglu" if g else ""), N=N, K=K, geglu=bool(g),
                  dt=DTYPES[(N // 8 + K + g) % 3]) for N in (5, 32, 64, 96) for K in (1, 8, 40) for g in (0, 1) if not (g and N % 32)]
PK_LINEAR_SECOND = Case(id="pk-lin-N2049-K1024-f16-second-trip", N=2049, K=1024, geglu=False, dt=F16)
PK_VEC = [Case(id="pk-vec-N%d-%s%s" % (N, DT_NAME[dt], "-geglu" if g else ""), N=N, geglu=g, dt=dt)
          for (N, g) in ((1, False), (257, False), (64, True), (96, True)) for dt in DTYPES]


def pack_source(c, shape):
    return odd_values(shape, c.dt, _gen("pk", c.id), 2.0)


def conv_w_shape(c):
    return (c.Cout, c.Cin) + {1: (1, 1), 3: (3, 1, 1), 9: (3, 3)}[c.taps]


def pack_conv_expect(w, planted=None):
    """[Cout][Cin][taps...] -> fp16 [Cout][taps][Cin]; planted taps_transposed: (ky, kx) read as (kx, ky)"""
    co, ci = w.shape[:2]
    if planted == "taps_transposed":
        w = w.transpose(2, 3)
    return w.reshape(co, ci, -1).permute(0, 2, 1).float().half().contiguous()


def pack_conv_dup_expect(w, planted=None):
    """fp16 [Cout][taps][2 Cin]: every tap's Cin weights twice; planted dup_shifted: the second half one channel on"""
    p = pack_conv_expect(w)
    second = torch.roll(p, 1, 2) if planted == "dup_shifted" else p
    return torch.cat([p, second], 2).contiguous()


def pack_direct_expect(w):
    """[Cout][Cin][3][3] -> fp32 [9][Cin][Cout]"""
    co, ci = w.shape[:2]
    return w.reshape(co, ci, 9).permute(2, 1, 0).float().contiguous()


PHASE_SETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def phase_sums(w, dtype=F32, planted=None):
    """[Cout][Cin][3][3] -> [4 = 2a + b][Cout][4 = 2ty + tx][Cin] in `dtype`: the sum over ky in S(a, ty), kx in S(b, tx) in (ky, kx) order.
    planted sets_swapped: S(0, 1) and S(1, 0) exchanged"""
    S = dict(PHASE_SETS)
    if planted == "sets_swapped":
        S[(0, 1)], S[(1, 0)] = S[(1, 0)], S[(0, 1)]
    co, ci = w.shape[:2]
    out = torch.zeros(4, co, 4, ci, dtype=dtype)
    wf = w.to(dtype)
    for a in (0, 1):
        for b in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    s = torch.zeros(co, ci, dtype=dtype)
                    for ky in S[(a, ty)]:
                        for kx in S[(b, tx)]:
                            s = s + wf[:, :, ky, kx]
                    out[2 * a + b, :, 2 * ty + tx] = s
    return out


def pack_phase_expect(w, planted=None):
    return phase_sums(w, F32, planted).half()


def geglu_row(p, N, planted=None):
    """packed row p -> source row; planted gate_from_32b: the gate rows taken from N/2 + 32 blk"""
    blk, wi = p >> 5, p & 31
    if wi < 16:
        return blk * 16 + wi
    return N // 2 + (32 if planted == "gate_from_32b" else 16) * blk + (wi - 16)


def pack_linear_expect(w, geglu, planted=None):
    N = w.shape[0]
    if geglu:
        w = w[[geglu_row(p, N, planted) % N for p in range(N)]]
    return w.float().half().contiguous()


def pack_vec_expect(v, geglu):
    N = v.shape[0]
    if geglu:
        v = v[[geglu_row(p, N) for p in range(N)]]
    return v.float().contiguous()


# ---- the fp16 range guard ----
OVF_KINDS = ("conv", "dup", "phase", "linear")
OVF_VALUES = {F32: ((65504.0, 0), (-65504.0, 0), (65505.0, 1), (65519.0, 1), (float("inf"), 1), (float("nan"), 1), (-7.0e4, 1)),
              BF16: ((65280.0, 0), (65536.0, 1), (-65536.0, 1), (float("inf"), 1), (float("nan"), 1))}
OVF_SECOND = {"conv": (257, 1024, 9), "dup": (129, 1024, 9), "phase": (129, 1024, 9), "linear": (2049, 1024, 1)}          # (rows, Cin | K, taps)
OVF_SMALL = {"conv": (5, 3, 9), "dup": (5, 3, 9), "phase": (5, 3, 9), "linear": (5, 40, 1)}


# the plan-level test: the smallest plan the suite builds (the tiny KL-VAE encoder of tests/vae_encoder_ref.py), one element of this fp32
# weight (a 3x3 GEMM convolution, packed by op_pack_conv_w with the plan's flag) at 7e4 / at 65504
PLAN_WEIGHT = "encoder.down_blocks.0.resnets.0.conv2.weight"


def ovf_work_items(kind, shape):
    r, c, t = shape
    return {"conv": r * c * t, "dup": 2 * r * c * t, "phase": 16 * r * c, "linear": r * c}[kind]


def ovf_source(kind, shape, dt, value, where):
    """a weight of small values (|w| <= 1) with `value` at flat source index 0 (`first`), the last (`last`) or the first element of the last
    output row (`second`: beyond the first grid-stride trip for the OVF_SECOND shapes); `value` None: nothing planted"""
    r, c, t = shape
    w = ((torch.arange(r * c * t, dtype=torch.int64) * 37 % 129).float() / 128.0 - 0.5).to(dt)
    if value is not None:
        # (the phase pack reads a source element into several outputs; the last one feeds the last output alone)
        idx = {"first": 0, "last": r * c * t - 1, "second": r * c * t - 1 if kind == "phase" else (r - 1) * c * t}[where]
        if kind == "phase":          # the planted tap alone in its 3x3 window: every phase sum it enters is the value itself
            w[idx // 9 * 9:idx // 9 * 9 + 9] = 0.0
        w[idx] = value
    return w.reshape((r, c, 3, 3) if t == 9 else (r, c))


def ovf_expected(kind, w, planted=None):
    """the flag, from the fp32 values the packer stores (the phase pack: its fp32 sums); planted last_missed: the last source element unseen"""
    w = w.float().clone()
    if planted == "last_missed":
        w.view(-1)[-1] = 0.0
    v = phase_sums(w, F32).reshape(-1) if kind == "phase" else w.reshape(-1)
    return int(bool((~(v.abs() <= FP16_MAX)).any()))


def ovf_phase_sum_source(dt):
    """every tap fits fp16 (4.0e4 each), the two-tap and four-tap phase sums do not: dup packs it clean, the phase pack flags it"""
    w = torch.full((2, 3, 3, 3), 0.25)
    w[1, 2] = 4.0e4
    return w.to(dt)


# ---------------------------------------------------------------------------------------------------------------------------
# unet_conv_out
# ---------------------------------------------------------------------------------------------------------------------------
CO_CS, CO_COUTS = (16, 24, 32, 40, 320), (1, 2, 3, 4)
CO_MAPS = ((1, 1), (1, 7), (7, 1), (5, 7), (8, 8))          # (H, W)
NCHW, NCFHW, ROWS = 0, 1, 2
CONV_OUT = []
for _i, (_C, _Co, (_H, _W)) in enumerate((c, o, m) for c in CO_CS for o in CO_COUTS for m in CO_MAPS):
    _lay, _N, _F = ((NCHW, 3, 1), (NCFHW, 6, 3), (ROWS, 3, 1), (NCFHW, 6, 1))[(_i + _i // 5) % 4]
    if (_H, _W) == (8, 8):
        _N = 6 if _lay == NCFHW else 2          # 128 or 384 pixels: exact multiples of 64
    _dt = DTYPES[(_i + _i // 3) % 3]
    CONV_OUT.append(Case(id="co-C%d-Co%d-%dx%d-N%d-%s%s-%s" % (_C, _Co, _H, _W, _N, ("nchw", "ncfhw", "rows")[_lay], "-F%d" % _F if _lay == NCFHW else "",
                                                             DT_NAME[_dt]), C=_C, Cout=_Co, H=_H, W=_W, N=_N, layout=_lay, F=_F, dt=_dt))
CONV_OUT.append(Case(id="co-C16-Co4-5x7-N3-rows-f32-i2v", C=16, Cout=4, H=5, W=7, N=3, layout=ROWS, F=1, dt=F32))          # I2VGen-XL's 16 -> 4 stem
CO_BY_ID = {c.id: c for c in CONV_OUT}


def conv_out_layout(y, c, planted=None):
    """y [N][Cout][H][W] -> the layout of the case; planted ncfhw_as_nchw"""
    if c.layout == ROWS:
        return y.permute(0, 2, 3, 1).contiguous()
    if c.layout == NCFHW and planted != "ncfhw_as_nchw":
        return y.reshape(c.N // c.F, c.F, c.Cout, c.H, c.W).permute(0, 2, 1, 3, 4).contiguous()
    return y.contiguous()


@functools.lru_cache(maxsize=None)
def conv_out_problem(case_id):
    """x fp16 [N][H][W][C], w fp32 [Cout][C][3][3], bias [Cout], ref, bound in the case's layout (fp64)"""
    c = CO_BY_ID[case_id]
    g = _gen("co", case_id)
    x = torch.randn(c.N, c.H, c.W, c.C, generator=g).half()
    w = torch.randn(c.Cout, c.C, 3, 3, generator=g) / math.sqrt(9.0 * c.C)
    b = torch.randn(c.Cout, generator=g)
    xc = x.double().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xc, w.double(), b.double(), padding=1)
    mag = torch.nn.functional.conv2d(xc.abs(), w.double().abs(), b.double().abs(), padding=1)
    bound = (9 * c.C + 8) * U * mag + quantum(ref, c.dt)
    return x, w, b, conv_out_layout(ref, c), conv_out_layout(bound, c)


def conv_out_emulate(case_id, planted=None):
    """lane q of a pixel: taps in order, its chunks q, q + 4, ..., eight fmas per output each; the lanes meet by xor 1, then xor 2.
    planted drop_last_lane: the last lane that owns a chunk (at C = 24 the third of the four) adds nothing; ncfhw_as_nchw"""
    c = CO_BY_ID[case_id]
    x, w, b, _, _ = conv_out_problem(case_id)
    xp = torch.nn.functional.pad(x.float(), (0, 0, 1, 1, 1, 1))          # [N][H + 2][W + 2][C]
    acc = torch.zeros(CO_LANES, c.N, c.H, c.W, c.Cout)
    for tap in range(9):
        xs = xp[:, tap // 3:tap // 3 + c.H, tap % 3:tap % 3 + c.W]
        for q in range(CO_LANES):
            if planted == "drop_last_lane" and q == min(CO_LANES, c.C // 8) - 1:
                continue
            for ch in range(q * 8, c.C, 32):
                for j in range(8):
                    acc[q] = NF._fma(w[:, ch + j, tap // 3, tap % 3].float()[None, None, None, :], xs[..., ch + j, None], acc[q])
    a = (acc[0] + acc[1]) + (acc[2] + acc[3])
    return conv_out_layout((a + b).permute(0, 3, 1, 2), c, planted).to(c.dt)


# ---------------------------------------------------------------------------------------------------------------------------
# i2v_frames
# ---------------------------------------------------------------------------------------------------------------------------
I2V = [Case(id="i2v-B%d-F%d-HW%d-%s" % (B, F, HW, DT_NAME[dt]), B=B, F=F, HW=HW, dt=dt) for B in (1, 2) for F in (1, 3) for HW in (1, 255, 257) for dt in DTYPES]


def i2v_problem(c):
    """x [B][4][F][HW] of c.dt, want fp32 [B F][4][HW]"""
    x = odd_values((c.B, 4, c.F, c.HW), c.dt, _gen("i2v", c.id))
    return x, x.float().permute(0, 2, 1, 3).reshape(c.B * c.F, 4, c.HW).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# vae_conv_in
# ---------------------------------------------------------------------------------------------------------------------------
CONV_IN = [Case(id="ci-%dx%d-Co%d-%s" % (H, W, Co, DT_NAME[dt]), H=H, W=W, Cout=Co, dt=dt)
           for (H, W) in ((1, 1), (1, 5), (7, 3), (17, 19)) for Co in (16, 48, 128) for dt in DTYPES]
CI_BY_ID = {c.id: c for c in CONV_IN}


@functools.lru_cache(maxsize=None)
def conv_in_problem(case_id):
    """px [3][H][W] of c.dt, w fp32 [Cout][3][3][3], b [Cout], ref, bound fp64 [H W][Cout]"""
    c = CI_BY_ID[case_id]
    g = _gen("ci", case_id)
    px = odd_values((3, c.H, c.W), c.dt, g, 1.0)
    w = torch.randn(c.Cout, 3, 3, 3, generator=g) / math.sqrt(27.0)
    b = torch.randn(c.Cout, generator=g)
    ref = torch.nn.functional.conv2d(px.double()[None], w.double(), b.double(), padding=1)[0]
    mag = torch.nn.functional.conv2d(px.double().abs()[None], w.double().abs(), b.double().abs(), padding=1)[0]
    f = lambda t: t.permute(1, 2, 0).reshape(c.H * c.W, c.Cout)
    return px, w, b, f(ref), f((27 + 2) * U * mag)


def conv_in_emulate(case_id, planted=None):
    """acc = bias, then 27 fmas in (tap, ci) order; planted last_group_unwritten"""
    c = CI_BY_ID[case_id]
    px, w, b, _, _ = conv_in_problem(case_id)
    xp = torch.nn.functional.pad(px.float(), (1, 1, 1, 1))
    acc = b[None, None, :].expand(c.H, c.W, c.Cout).clone()
    for tap in range(9):
        for ci in range(3):
            acc = NF._fma(w[:, ci, tap // 3, tap % 3][None, None, :], xp[ci, tap // 3:tap // 3 + c.H, tap % 3:tap % 3 + c.W, None], acc)
    acc = acc.reshape(c.H * c.W, c.Cout)
    if planted == "last_group_unwritten":
        acc[-1, -CI_GROUP:] = POISON[F32]
    return acc


# ---------------------------------------------------------------------------------------------------------------------------
# vae_row_softmax
# ---------------------------------------------------------------------------------------------------------------------------
SM_LS = (1, 63, 255, 256, 257, 1000)
SM_KINDS = ("plain", "constant", "spike_first", "spike_last", "step")
SOFTMAX = []
for _i, _L in enumerate(SM_LS):
    for _j, _Lp in enumerate((_L, -(-_L // 64) * 64, _L + 300)):
        for _k, _kind in enumerate(SM_KINDS):
            SOFTMAX.append(Case(id="sm-L%d-Lpad%d-rows%d-%s" % (_L, _Lp, (1, 3)[(_i + _j + _k) % 2], _kind), L=_L, Lpad=_Lp, rows=(1, 3)[(_i + _j + _k) % 2],
                                kind=_kind))
SM_BY_ID = {c.id: c for c in SOFTMAX}


@functools.lru_cache(maxsize=None)
def softmax_problem(case_id):
    """S [rows][L] fp32, ref, bound fp64 [rows][L], exact (fp16 [rows][L] the result must equal bit for bit, or None)"""
    c = SM_BY_ID[case_id]
    g = _gen("sm", c.L, c.rows, c.kind)
    exact = None
    if c.kind == "plain":
        S = torch.randn(c.rows, c.L, generator=g) * 6.0
    elif c.kind == "step":          # the entries from 256 on (L <= 256: from L / 2 on) lie 120 higher: exp(120) overflows fp32, so a maximum
        S = torch.randn(c.rows, c.L, generator=g)          # that misses them shows; the low entries underflow to exactly 0
        S[:, (SM_THREADS if c.L > SM_THREADS else c.L // 2):] += 120.0
    elif c.kind == "constant":
        S = (torch.randn(c.rows, 1, generator=g) * 6.0).expand(c.rows, c.L).contiguous()
        exact = torch.full((c.rows, c.L), 1.0 / c.L, dtype=torch.float64).half()
    else:
        S = torch.randn(c.rows, c.L, generator=g).clamp(-4.0, 4.0)
        at = 0 if c.kind == "spike_first" else c.L - 1
        S[:, at] = S.max(1).values + 80.0 if c.L > 1 else S[:, at]
        exact = torch.zeros(c.rows, c.L, dtype=F16)
        exact[:, at] = 1.0
    s64 = S.double()
    d = s64 - s64.max(1, keepdim=True).values
    ref = torch.softmax(s64, 1)
    bound = NF.ulp16(ref) + softmax_term(S)
    return S, ref, bound, exact


def softmax_term(S):
    """the SM_K term alone (+ a flushed denormal): what the fp32 value before the store is held to when SM_K is calibrated"""
    s64 = S.double()
    d = s64 - s64.max(1, keepdim=True).values
    return SM_K * U * torch.softmax(s64, 1) * (1.0 + d.abs()) + 2.0 ** -126


def softmax_emulate(case_id, planted=None, keep32=False):
    """thread t walks c = t, t + 256, ...; wave butterfly; (red0 + red1) + (red2 + red3); p = fp16(expf(s - m) * (1 / z)).
    planted max_first_256: the maximum over the first 256 entries only; keep32: the fp32 value before the store (what SM_K is calibrated on)"""
    c = SM_BY_ID[case_id]
    S, _, _, _ = softmax_problem(case_id)
    m = (S[:, :SM_THREADS] if planted == "max_first_256" else S).max(1, keepdim=True).values
    e = torch.exp(S - m)
    trips = -(-c.L // SM_THREADS)
    ep = NF._pad(e, 1, trips * SM_THREADS).reshape(c.rows, trips, 4, 64)
    z = NF._seq_sum(ep, 1)
    zw = NF._xor_tree(z, 64)
    zt = (zw[:, 0] + zw[:, 1]) + (zw[:, 2] + zw[:, 3])
    p = e * (torch.tensor(1.0, dtype=F32) / zt)[:, None]
    return p if keep32 else p.half()


def softmax_share(out, ref, bound):
    """the share of the calibrated term once the half quantum a correct rounding costs is taken off"""
    q = NF.ulp16(ref)
    o = out.double()
    if not bool(torch.isfinite(o).all()):
        return float("inf")
    return float((((o - ref).abs() - 0.5 * q) / (bound - q)).max().clamp_min(0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# what the entry points refuse before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(ptr, odd_ptr):
    """[(name, symbol, ctypes argument list without the stream, part of the message)]: `ptr` any 16-byte aligned address the call may
    name (a refused call dereferences nothing), `odd_ptr` one that is 2 mod 16.  The stream goes last on every entry point."""
    import ctypes as C
    P, I, Q, Z, F = (lambda: C.c_void_p(ptr)), C.c_int, C.c_int64, C.c_size_t, C.c_float
    null = C.c_void_p(0)
    m17, p9, i9 = (C.c_int * 17)(*([1] * 17)), (C.c_void_p * 9)(*([ptr] * 9)), (C.c_int * 9)(*range(9))
    rows = [
        ("avgpool 6x4 -> 4x4", "ctrl_avgpool_nchw", [P(), P(), I(1), I(1), I(6), I(4), I(4), I(4)], "avgpool: only integer pooling ratios"),
        ("sincos odd dim", "ctrl_op_timestep_sincos", [P(), I(1), P(), I(1), I(5)], "dim must be even"),
        ("sincos 2 of 3 timesteps", "ctrl_op_timestep_sincos", [P(), I(2), P(), I(3), I(6)], "need 1 or N timesteps"),
        ("linear_small K = 12", "ctrl_op_linear_small", [P(), Q(16), P(), null, P(), Q(4), I(1), I(4), I(12), I(0), I(0)], "K must be a multiple of 8"),
        ("linear_small ldx = 6", "ctrl_op_linear_small", [P(), Q(6), P(), null, P(), Q(4), I(1), I(4), I(8), I(0), I(0)], "ldx of 4"),
        ("blend bf16", "ctrl_op_blend", [P(), I(1), P(), I(2), P(), P(), I(1), Z(8)], "blend: fp16 / fp32 only"),
        ("blend n = 12", "ctrl_op_blend", [P(), I(1), P(), I(1), P(), P(), I(1), Z(12)], "multiple of 8"),
        ("merge K = 0", "ctrl_router_merge", [p9, P(), i9, I(0), P(), I(1), Z(8)], "1..8 experts"),
        ("merge K = 9", "ctrl_router_merge", [p9, P(), i9, I(9), P(), I(1), Z(8)], "1..8 experts"),
        ("router E = 17", "ctrl_router_weights", [P(), m17, P(), I(1), I(17), I(0)], "1..16 experts"),
        ("pack_vec geglu N = 48", "ctrl_op_pack_vec", [P(), I(0), P(), I(48), I(1)], "pack_vec: GEGLU needs N % 32 == 0"),
        ("pack_linear_w geglu N = 48", "ctrl_op_pack_linear_w", [P(), I(0), P(), I(48), I(8), I(1)], "pack_linear_w: GEGLU needs N % 32 == 0"),
        ("pack_vec null", "ctrl_op_pack_vec", [null, I(0), P(), I(8), I(0)], "pack_vec: null pointer"),
        ("pack_vec N = 0", "ctrl_op_pack_vec", [P(), I(0), P(), I(0), I(0)], "pack_vec: every extent"),
        ("pack_linear_w null out", "ctrl_op_pack_linear_w", [P(), I(0), null, I(8), I(8), I(0)], "pack_linear_w: null pointer"),
        ("pack_linear_w dtype 3", "ctrl_op_pack_linear_w_ovf", [P(), I(3), P(), I(8), I(8), I(0), P()], "pack_linear_w: the source must be"),
        ("pack_conv_w null", "ctrl_op_pack_conv_w", [null, I(0), P(), I(1), I(1), I(9)], "pack_conv_w: null pointer"),
        ("pack_conv_w taps = 0", "ctrl_op_pack_conv_w_ovf", [P(), I(0), P(), I(1), I(1), I(0), P()], "pack_conv_w: every extent"),
        ("pack_conv_w too large", "ctrl_op_pack_conv_w", [P(), I(0), P(), I(65536), I(65536), I(9)], "pack_conv_w: too many elements"),
        ("pack_conv_w_dup Cin = -1", "ctrl_op_pack_conv_w_dup", [P(), I(0), P(), I(1), I(-1), I(9)], "pack_conv_w_dup: every extent"),
        ("pack_conv_w_dup null", "ctrl_op_pack_conv_w_dup_ovf", [P(), I(0), null, I(1), I(1), I(9), P()], "pack_conv_w_dup: null pointer"),
        ("pack_conv_w_phase Cout = 0", "ctrl_op_pack_conv_w_phase_ovf", [P(), I(0), P(), I(0), I(8), P()], "pack_conv_w_phase"),
        ("pack_conv_w_direct null", "ctrl_op_pack_conv_w_direct", [null, I(0), P(), I(1), I(1)], "pack_conv_w_direct: null pointer"),
        ("pack_conv_w_direct dtype -1", "ctrl_op_pack_conv_w_direct", [P(), I(-1), P(), I(1), I(1)], "pack_conv_w_direct: the source must be"),
        ("softmax Lpad < L", "ctrl_op_vae_row_softmax", [P(), Q(70), P(), Q(70), I(1), I(64), I(63)], "vae_row_softmax: bad shape"),
        ("softmax lds < L", "ctrl_op_vae_row_softmax", [P(), Q(63), P(), Q(70), I(1), I(64), I(64)], "vae_row_softmax: bad shape"),
        ("conv_in Cout = 8", "ctrl_op_vae_conv_in", [P(), I(0), P(), P(), P(), I(4), I(4), I(8)], "vae_conv_in: bad shape"),
        ("conv_in Cout = 24", "ctrl_op_vae_conv_in", [P(), I(0), P(), P(), P(), I(4), I(4), I(24)], "vae_conv_in: bad shape"),
        ("i2v_frames dtype 3", "ctrl_op_i2v_frames", [P(), I(3), P(), I(1), I(1), I(4)], "i2v_frames: image_latents must be"),
        ("i2v_frames F = 0", "ctrl_op_i2v_frames", [P(), I(0), P(), I(1), I(0), I(4)], "i2v_frames: bad arguments"),
    ]
    co = lambda x=None, C_=32, Cout=4, N=6, layout=NCHW, F=1: [x or P(), P(), P(), P(), I(0), I(N), I(2), I(2), I(C_), I(Cout), I(layout), I(F)]
    rows += [
        ("conv_out C = 8", "ctrl_op_unet_conv_out", co(C_=8), "unet_conv_out: C a multiple of 8 from 16"),
        ("conv_out C = 20", "ctrl_op_unet_conv_out", co(C_=20), "unet_conv_out: C a multiple of 8 from 16"),
        ("conv_out Cout = 5", "ctrl_op_unet_conv_out", co(Cout=5), "unet_conv_out: C a multiple of 8 from 16"),
        ("conv_out ncfhw N = 5 F = 3", "ctrl_op_unet_conv_out", co(N=5, layout=NCFHW, F=3), "unet_conv_out: bad output layout"),
        ("conv_out layout 3", "ctrl_op_unet_conv_out", co(layout=3), "unet_conv_out: bad output layout"),
        ("conv_out misaligned x", "ctrl_op_unet_conv_out", co(x=C.c_void_p(odd_ptr)), "unet_conv_out: x must be 16-byte aligned"),
    ]
    return rows
