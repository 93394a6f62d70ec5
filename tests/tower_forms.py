"""The kernels under the two CLIP towers (csrc/text_gemm.hip, csrc/text.hip, csrc/vision.hip) at their split, tile and row edges: case
tables, problem builders, fp64 references with element-wise bounds, fp32 emulations of the kernels' arithmetic in their own association and
the planted errors the bounds have to reject.  Pure data: imports no GPU code.

    GPU tests: tests/test_gpu_tower_forms.py        host self-test (no GPU): tests/test_tower_check_host.py

Few-row GEMM.  y = act(x W^T + b) (+ res), fp16 operands, fp32 accumulation; with u = 2^-24, mag = |x| |W|^T + |b| (+ |res|):
    act 0        helpers.igemm_bound(ref, mag, K): (K + 8) u mag in any order + one rounding of the stored value
    act 2, 3     igemm_bound(ref, slope * mag, K) + e_act(|v| + dv),  v the pre-activation, dv = (K + 8) u mag
      slope      1.13 for GELU (as tests/ffn_forms.py); 1.1 for x sigmoid(k x): d/dx = s + z s (1 - s), z = k x, whose maximum over z is
                 1.0998 whatever k (the host self-test evaluates it on a grid)
      e_quick    x_sigmoid_kx (csrc/common.h) = x * rcp(1 + __expf(-k x)), a = k |x|, s = sigmoid(k x):
                   the exponential's argument carries 4 roundings relative to a (the constant 1.702f, the product k x, the constant log2 e
                   and the product in front of v_exp_f32): 4 u a on e = exp(-k x); v_exp_f32 is good to 1 ulp = 2 u;
                   e enters s with the weight e / (1 + e) = 1 - s;
                   the sum 1 + e rounds once (u), v_rcp_f32 is good to 1 ulp (2 u), the product x * r rounds once (u):
                 |error| <= |x s| (4 u + (1 - s) (4 u a + 2 u)) + 2^-126     (2^-126: a flushed denormal)
      e_erf      0.5 v (1 + erff(v / sqrt 2)): no ulp figure of the device erff is at hand, so its constant is taken the way
                 tests/norm_forms.py takes GN_K: e_erf = ERF_K u |v| with ERF_K the smallest power of two for which the fp32 CPU
                 emulation stays at or below 0.5 of the bound on the finish-alone cases (exact pre-activation, so only the activation and
                 the store remain); the factor 2 is the margin for the device erff differing from the host's.
                 ERF_K = 2^2; measured share: 0.41 of the bound on this table (fp32 stores, act 3), 0.45 on a grid over
                 [-12, 12]; one power of two less gives 0.69 and 0.89.
                 Printed by tests/test_tower_check_host.py::test_emulations_stay_within_their_bounds.
    The finish kernel alone runs over planes of small dyadic values: the sum over the splits and the bias is exact, the bound is
    e_act + one rounding of the residual add (u (|act| + |res|)) + one rounding of the stored value.

Causal attention.  helpers.attn_reference with the causal mask, p_fp16 = True, c = scale * log2(e).  Data kinds: `plain`; `diagonal` (key i
    is 4 q_i: the last visible key of every query dominates its row); `future` (keys from position t on carry V = +-6e4 and a doubled K: K and
    V belong to a key, not to a (query, key) pair, so "the keys after the query" is realised per pair -- every query below t must not see
    them at all, the queries from t on see them legitimately and are held to the same bound; t is the second key of the last query tile for
    a single pair and walks over the positions with the pair index otherwise).

Row kernels.  The LayerNorm bound of tests/norm_forms.py (n = C, kappa = 1): quantum(ref) + K u (1 + log2 C) (|gamma| (1 + |xhat|) + |beta|),
    the quantum that of the output type.  norm_forms.LN_K = 2^-2 does NOT hold on this table: the criterion (the fp32 emulation in row_ln's
    own association -- per-thread strided sums, wave butterfly, four-wave sum -- at or below 0.5 of the bound) fails for `plain` at every
    width above 1 (share of the statistics term 0.56 to 0.87, the largest at C = 63): the emulation rounds every operation of the chain
    (x - mean) rstd gamma + beta on its own, as the kernel may, and these roundings do not shrink with C while 1 + log2 C does.  The next
    power of two holds: LN_K_PLAIN = 2^-1 (share 0.44).
    `offset` (row mean = 32 std) needs more: the two-pass statistics remove the cancellation of E[x^2] - mean^2 but not the rounding of
    the mean itself, which is relative to |mean| = 32 std and not to std -- the division sum / C alone may cost half an ulp of 32, i.e.
    2^-19 = 32 u on every xhat of the row.  The powers of two are taken until the criterion holds: LN_K_OFFSET = 2^5 (emulated share 0.27
    at C = 257; 2^4 gives 0.54).  `flat` (a dyadic constant: exact row sum, d = 0) must give beta
    rounded to the output type bit for bit.
"""
import functools
import math
import zlib

import torch

import helpers
import norm_forms as NF

U = 2.0 ** -24
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
DT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
EPS = 1e-5


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


class Case(dict):
    __getattr__ = dict.get

    def __hash__(self):
        return hash(self["id"])

    def __eq__(self, other):
        return self is other


def quantum(ref, dt):
    """one quantum of the output type at |ref| (fp16: norm_forms.ulp16)"""
    if dt == F16:
        return NF.ulp16(ref)
    mant = 23 if dt == F32 else 7
    _, e = torch.frexp(ref.abs().double().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 1 - mant)


def store_round(ref, dt):
    """one round-to-nearest of the stored value, as helpers.igemm_bound counts it (fp32: the value is the fp32 result itself)"""
    if dt == F16:
        return 2.0 ** -11 * ref.abs() + 2.0 ** -25
    if dt == BF16:
        return 2.0 ** -8 * ref.abs()
    return torch.zeros_like(ref)


def check(out, ref, bound):
    """worst |out - ref| / bound (fp64); inf when an output is not finite"""
    o = out.double()
    if not bool(torch.isfinite(o).all()):
        return float("inf")
    return float(((o - ref).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------
QUICK_K = 1.702
SLOPE = {0: 1.0, 2: 1.1, 3: 1.13}
ERF_K = 2.0 ** 2


def act64(v, act):
    if act == 2:
        return v * torch.sigmoid(QUICK_K * v)
    if act == 3:
        return 0.5 * v * (1.0 + torch.special.erf(v / math.sqrt(2.0)))
    return v


def act_err(v_abs_hi, v, act, erf_k=ERF_K):
    """the activation's own error at a pre-activation v known to |v| <= v_abs_hi (header: e_quick, e_erf)"""
    if act == 0:
        return torch.zeros_like(v)
    if act == 3:
        return erf_k * U * v_abs_hi
    a = QUICK_K * v_abs_hi
    s = torch.sigmoid(QUICK_K * v)
    return v_abs_hi * s * (4 * U + (1 - s) * (4 * U * a + 2 * U)) + 2.0 ** -126


def act_emul(v, act):
    """fp32 restatement of apply_act (csrc/text_gemm.hip), exp and rcp correctly rounded, erf the host's"""
    v = v.float()
    if act == 2:
        return v * (1.0 / (1.0 + torch.exp(-(torch.tensor(QUICK_K, dtype=F32) * v))))
    if act == 3:
        return torch.tensor(0.5, dtype=F32) * v * (1.0 + torch.erf(v * torch.tensor(0.70710678118654752, dtype=F32)))
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# few-row GEMM (csrc/text_gemm.hip)
# ---------------------------------------------------------------------------------------------------------------------------
TG_WAVES, TG_KW, TG_KS, TG_BN, TG_ROWS = 4, 128, 512, 32, 32          # kTgWaves, kTgKW, kTgKS, kTgBN, kTgRows
GEMM_NK = ((16, 32), (48, 96), (32, 128), (32, 160), (32, 512), (32, 544), (48, 1056), (64, 992), (80, 1280),
           (32, 320))          # (32, 320): the one K with K % 128 == 64, a wave of two k-steps
GEMM_MS = (1, 15, 16, 17, 31, 32, 33, 65, 77)
GEMM_ALL_M = ((48, 1056), (32, 160))          # every M runs with these two: a half-filled tile over three splits, and two waves, one of one step
GEMM_MAXM = 77


def gemm_geometry(N, K):
    """restated from text_gemm_partial_kernel: splits and, per split, (nwaves, [nsteps of waves 0..3])"""
    splits = -(-K // TG_KS)
    out = []
    for s in range(splits):
        nwaves = min(TG_WAVES, (K - s * TG_KS + TG_KW - 1) // TG_KW)
        nsteps = [min(max((K - (s * TG_KS + w * TG_KW)) // 32, 0), TG_KW // 32) for w in range(TG_WAVES)]
        out.append((nwaves, nsteps))
    return splits, out


def _gemm_table():
    pairs = [(nk, M) for nk in GEMM_NK for M in (33, 77)] + [(nk, M) for nk in GEMM_ALL_M for M in GEMM_MS if M not in (33, 77)]
    cases = []
    for i, ((N, K), M) in enumerate(pairs):
        act = (0, 2, 3)[i % 3]
        dt = DTYPES[(i // 3 + i) % 3]
        bias = i % 4 != 1
        res = i % 5 in (0, 3)
        cases.append(Case(id="N%d-K%d-M%d-act%d-%s%s%s" % (N, K, M, act, DT_NAME[dt], "" if bias else "-nobias", "-res" if res else ""),
                          N=N, K=K, M=M, act=act, dt=dt, bias=bias, res=res))
    return cases


GEMM = _gemm_table()
GEMM_BY_ID = {c.id: c for c in GEMM}


@functools.lru_cache(maxsize=None)
def gemm_operands(N, K):
    """x [77][K] fp16, W [N][K] fp16, bias [N] fp32, res [77][N] fp32 of an (N, K): a case of M rows takes the first M rows, so the rows of
    different M are the same problem (batch invariance)"""
    g = _gen("tgemm", N, K)
    x = torch.randn(GEMM_MAXM, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) * (1.5 / math.sqrt(K))).half()
    return x, W, torch.randn(N, generator=g), torch.randn(GEMM_MAXM, N, generator=g)


@functools.lru_cache(maxsize=None)
def gemm_reference(case_id):
    """(ref, bound) fp64 [M][N]"""
    c = GEMM_BY_ID[case_id]
    x, W, b, r = gemm_operands(c.N, c.K)
    x, W = x[:c.M].double(), W.double()
    v = x @ W.t()
    mag = x.abs() @ W.abs().t()
    if c.bias:
        v, mag = v + b.double(), mag + b.double().abs()
    dv = (c.K + 8) * U * mag
    ref = act64(v, c.act)
    if c.res:
        ref, mag = ref + r[:c.M].double(), mag + r[:c.M].double().abs()
    bound = helpers.igemm_bound(ref, mag * SLOPE[c.act], c.K, 1.0, c.dt) + act_err(v.abs() + dv, v, c.act)
    return ref, bound


GEMM_PLANTED = ("drop_last_kstep_of_partial_wave", "nwaves_minus_one", "nwaves_plus_one", "drop_last_split", "zero_upper_half_tile",
                "tail_rows_reuse_last")


def gemm_emulate(case_id, planted=None):
    """the kernel's arithmetic in fp32 on the CPU: a wave adds its k-steps of 32 in order (each an fp32 dot product), the waves are added
    in wave order, the splits in split order, then bias, activation, residual and the store.
    Planted errors: a wave with fewer than four k-steps drops its last; the wave sum runs over nwaves - 1 slots (the first slot is always
    read); over nwaves + 1 slots (a wave without k-steps wrote zeros, so this shows only where all four waves are live: the fifth slot lies
    past the array and is modelled as an alias of slot 0); the last split is left out; the upper 16 columns of a half-filled column tile
    are zero; every row of the last, partial 32-row pass holds row M - 1."""
    c = GEMM_BY_ID[case_id]
    x, W, b, r = gemm_operands(c.N, c.K)
    x, W = x[:c.M].float(), W.float()
    splits, geo = gemm_geometry(c.N, c.K)
    total = None
    for s in range(splits - (1 if planted == "drop_last_split" and splits > 1 else 0)):
        nwaves, nsteps = geo[s]
        parts = []
        for w in range(TG_WAVES):
            n = nsteps[w]
            if planted == "drop_last_kstep_of_partial_wave" and 0 < n < TG_KW // 32:
                n -= 1
            acc = torch.zeros(c.M, c.N)
            for ks in range(n):
                k0 = s * TG_KS + w * TG_KW + ks * 32
                acc = acc + x[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
            parts.append(acc)
        nw = nwaves + {"nwaves_minus_one": -1, "nwaves_plus_one": 1}.get(planted, 0)
        tot = parts[0]
        for w in range(1, nw):
            tot = tot + parts[w % TG_WAVES]
        total = tot if total is None else total + tot
    if planted == "zero_upper_half_tile" and c.N % TG_BN == 16:
        total = total.clone()
        total[:, c.N - 16:] = 0.0
    if c.bias:
        total = total + b
    y = act_emul(total, c.act)
    if c.res:
        y = y + r[:c.M]
    if planted == "tail_rows_reuse_last":
        r0 = (c.M - 1) // TG_ROWS * TG_ROWS
        y = y.clone()
        y[r0:] = y[c.M - 1]
    return y.to(c.dt)


# the finish kernel alone: planes of small dyadic values, ldres = N + 4, ldy = N + 8
FIN_GRID_BLOCKS, FIN_THREADS = 8192, 256          # op_text_gemm_finish: at most 8192 workgroups of 256, four columns per thread
FINISH = []
for _i, (_M, _N) in enumerate(((5, 20), (33, 48), (3, 4))):
    for _s in (1, 2, 3):
        for _act in (0, 2, 3):
            _k = len(FINISH)
            _dt = DTYPES[(_k + _i) % 3] if not (_act == 3 and _s == 1) else F32
            FINISH.append(Case(id="fin-M%d-N%d-s%d-act%d-%s%s" % (_M, _N, _s, _act, DT_NAME[_dt], "-res" if _k % 2 == 0 else ""),
                               M=_M, N=_N, splits=_s, act=_act, dt=_dt, bias=_k % 3 != 2, res=_k % 2 == 0))
# M N / 4 just above 8192 * 256 with one plane: the second trip of the grid-stride loop
FINISH.append(Case(id="fin-M1648-N5120-s1-act2-f16-second-trip", M=1648, N=5120, splits=1, act=2, dt=F16, bias=True, res=False))
FIN_BY_ID = {c.id: c for c in FINISH}


@functools.lru_cache(maxsize=4)
def finish_problem(case_id):
    """ws [splits][M][N] fp32 (multiples of 1/8 in [-4, 4)), bias [N] | None (multiples of 1/4), res [M][N] fp32 | None, ref, bound"""
    c = FIN_BY_ID[case_id]
    g = _gen("tfin", case_id)
    ws = (torch.randint(-32, 32, (c.splits, c.M, c.N), generator=g).float() / 8.0)
    bias = torch.randint(-8, 8, (c.N,), generator=g).float() / 4.0 if c.bias else None
    res = torch.randn(c.M, c.N, generator=g) if c.res else None
    v = ws.double().sum(0) + (bias.double() if c.bias else 0.0)          # exact in fp32 as well
    a = act64(v, c.act)
    ref = a if res is None else a + res.double()
    bound = act_err(v.abs(), v, c.act) + store_round(ref, c.dt) + 2.0 ** -140
    if res is not None:
        bound = bound + U * (a.abs() + res.double().abs())
    return dict(ws=ws, bias=bias, res=res, ref=ref, bound=bound, v=v)


def finish_emulate(case_id):
    c = FIN_BY_ID[case_id]
    p = finish_problem(case_id)
    v = p["ws"][0]
    for s in range(1, c.splits):
        v = v + p["ws"][s]
    if c.bias:
        v = v + p["bias"]
    y = act_emul(v, c.act)
    if c.res:
        y = y + p["res"]
    return y.to(c.dt)


# ---------------------------------------------------------------------------------------------------------------------------
# causal attention (csrc/text.hip: text_attn_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
ATTN_LS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 77, 96, 97, 112, 113, 127, 128)
ATTN_PAIRS = ((1, 1), (7, 1), (4, 2), (3, 3), (1, 20), (2, 20))          # (N, heads): 1, 7, 8, 9, 20 and 40 (prompt, head) pairs
ATTN_STRIDES = ((0, 0), (8, 0), (0, 16), (8, 16))          # (ld - 3 C, ldo - C)
ATTN_KINDS = ("plain", "diagonal", "future")
ATTN_SCALE = 0.125
ATTN_C = ATTN_SCALE * 1.4426950408889634


def attn_geometry(L):
    """restated from op_text_attn / text_attn_kernel: kpad, and per query tile (nk, nkt, nkp)"""
    kpad = (L + 31) & ~31
    tiles = []
    for qt in range((L + 15) // 16):
        nk = min(L, qt * 16 + 16)
        tiles.append((nk, (nk + 15) >> 4, (nk + 31) & ~31))
    return kpad, tiles


def _attn_table():
    cases = []
    for i, L in enumerate(ATTN_LS):
        cases.append((L, 1, 1, 0, 0, ATTN_KINDS[i % 3]))
    k = 0
    for L in (17, 77, 128):
        for (N, heads) in ATTN_PAIRS:
            for (dl, do) in ATTN_STRIDES:
                cases.append((L, N, heads, dl, do, ATTN_KINDS[k % 3]))
                k += 1
    return [Case(id="L%d-N%d-h%d-ld+%d-ldo+%d-%s" % c, L=c[0], N=c[1], heads=c[2], dld=c[3], dldo=c[4], kind=c[5]) for c in cases]


ATTN = _attn_table()
ATTN_BY_ID = {c.id: c for c in ATTN}


def future_start(L, pair, pairs):
    """first position of the large keys of a `future` pair (L when there is none)"""
    if L == 1:
        return L
    if pairs == 1:
        q0 = 16 * ((L - 1) // 16)
        if L - 1 > q0:
            return q0 + 1
        return q0 - 15 if q0 > 0 else L
    return 1 + (5 * pair) % (L - 1)


def attn_qkv(kind, L, N, heads, seed=0):
    """q, k, v fp16 [N][heads][L][64]; prompt n's data depends on (kind, L, heads, seed, n) alone"""
    q = torch.empty(N, heads, L, 64, dtype=F16)
    k, v = torch.empty_like(q), torch.empty_like(q)
    for n in range(N):
        g = _gen("tattn", kind, L, heads, seed, n)
        qn, kn, vn = (torch.randn(heads, L, 64, generator=g) for _ in range(3))
        if kind == "diagonal":
            kn = 4.0 * qn
        elif kind == "future":
            for h in range(heads):
                t = future_start(L, n * heads + h, N * heads)
                kn[h, t:] *= 2.0
                vn[h, t:] = torch.where(vn[h, t:] >= 0, 6.0e4, -6.0e4)
        q[n], k[n], v[n] = qn.half(), kn.half(), vn.half()
    return q, k, v


@functools.lru_cache(maxsize=8)
def attn_problem(case_id):
    c = ATTN_BY_ID[case_id]
    q, k, v = attn_qkv(c.kind, c.L, c.N, c.heads)
    ref, bound = attn_ref(q, k, v)
    return dict(q=q, k=k, v=v, ref=ref, bound=bound)


def causal_mask(L):
    return torch.ones(L, L, dtype=torch.bool).tril()


def attn_ref(q, k, v):
    """(ref, bound) fp64 [N][heads][L][64] of the causal attention"""
    N, H, L, D = q.shape
    f = lambda t: t.reshape(N * H, L, D)
    ref, bound = helpers.attn_reference(f(q), f(k), f(v), ATTN_C, p_fp16=True, mask=causal_mask(L))
    return ref.reshape(N, H, L, D), bound.reshape(N, H, L, D)


def attn_pack(q, k, v, ld):
    """the Q | K | V GEMM output [N*L][ld] fp16 (pad columns NaN)"""
    N, H, L, D = q.shape
    C = H * D
    out = torch.full((N * L, ld), float("nan"), dtype=F16)
    for j, t in enumerate((q, k, v)):
        out[:, j * C:(j + 1) * C] = t.permute(0, 2, 1, 3).reshape(N * L, C)
    return out


def attn_unpack(out, N, heads, L):
    """[N*L][>= C] -> [N][heads][L][64]"""
    return out[:, :heads * 64].reshape(N, L, heads, 64).permute(0, 2, 1, 3)


ATTN_PLANTED = ("mask_key_lt_q", "mask_off_past_L", "p_not_zeroed")


def attn_emulate(q, k, v, planted=None):
    """text_attn_kernel in fp32 on the CPU: S and O as fp32 products, the mask before the row max, P rounded to fp16, the row sum over the
    fp32 values.  Planted errors: the mask is key < q; the keys between L and the end of the last 16-key tile (zero rows of K and V in
    LDS) are visible to every query; the P columns between the last score tile and the 32-key extent of P V are not zeroed (uninitialised
    LDS, modelled as NaN)."""
    N, H, L, D = q.shape
    Lp = (L + 15) & ~15
    pad = lambda t: torch.cat([t.float(), torch.zeros(N, H, Lp - L, D)], 2)
    kf, vf = pad(k), pad(v)
    s = (q.float() @ kf.transpose(-1, -2)) * torch.tensor(ATTN_C, dtype=F32)
    qi, ki = torch.arange(L)[:, None], torch.arange(Lp)[None, :]
    vis = (ki < qi) if planted == "mask_key_lt_q" else (ki <= qi)
    vis = vis & (ki < L)
    if planted == "mask_off_past_L":
        vis = vis | (ki >= L)
    s = torch.where(vis, s, torch.tensor(float("-inf")))
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = p.half().float() @ vf
    out = o * (1.0 / p.sum(-1, keepdim=True))
    if planted == "p_not_zeroed":
        _, tiles = attn_geometry(L)
        for qt, (nk, nkt, nkp) in enumerate(tiles):
            if nkt * 16 < nkp:
                out[:, :, qt * 16:qt * 16 + 16] = float("nan")
    return out.half()


# ---------------------------------------------------------------------------------------------------------------------------
# row kernels (csrc/text.hip, csrc/vision.hip)
# ---------------------------------------------------------------------------------------------------------------------------
ROW_CS = (1, 63, 64, 255, 256, 257, 1000, 1023, 1024, 1088, 1280, 2048)
ROW_KINDS = ("plain", "offset", "flat")
ROW_THREADS = 256
LN_K_PLAIN = 2.0 ** -1
LN_K_OFFSET = 2.0 ** 5
FLAT_VALUE = 1.5


def text_row_kernel(C, pooled32=False):
    """the kernel op_text_embed / op_text_final_ext launch for a width (None: refused)"""
    if C <= 1024:
        return ("text_final_ext<4>" if pooled32 else "text_final"), 4
    if C <= 2048 and C % 64 == 0:
        return "text_final_ext<8>", 8
    return None


def ln_k(kind):
    return LN_K_OFFSET if kind == "offset" else LN_K_PLAIN


def row_data(kind, rows, C, *key):
    """x [rows][C] fp32 (not fp16-representable), gamma, beta [C]"""
    g = _gen("trow", kind, rows, C, key)
    chan = torch.randn(C, generator=g)
    x = 0.5 + 0.9 * torch.randn(rows, C, generator=g) + 0.45 * chan
    if kind == "offset":
        x = x - 0.5 + 32.0 * math.sqrt(0.81 + 0.2025)
    elif kind == "flat":
        x = torch.full((rows, C), FLAT_VALUE)
    return x.float(), (1.0 + 0.3 * torch.randn(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()


def ln_ref(x, gamma, beta, dt, kind="plain"):
    """(ref, bound) fp64 of LayerNorm(x [rows][C]) stored as dt"""
    x = x.double()
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    d = x - mean
    xhat = d / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
    ref = xhat * gamma.double() + beta.double()
    stat = ln_k(kind) * U * (1.0 + math.log2(C)) * (gamma.double().abs() * (1.0 + xhat.abs()) + beta.double().abs())
    return ref, quantum(ref, dt) + stat


def ln_stat_share(out, x, gamma, beta, dt, kind):
    """the share of the statistics term an output uses once the half quantum of a correct rounding is taken off (norm_forms.stat_part)"""
    ref, bound = ln_ref(x, gamma, beta, dt, kind)
    q = quantum(ref, dt)
    err = (out.double() - ref).abs()
    return float(((err - 0.5 * q) / (bound - q)).max().clamp_min(0.0))


def _block_sum(t):
    """t [rows][PER][256] fp32 -> [rows]: the thread's values in order, the wave butterfly, the four waves in order"""
    acc = torch.zeros_like(t[:, 0])
    for i in range(t.shape[1]):
        acc = acc + t[:, i]
    w = NF._xor_tree(acc.reshape(-1, 4, 64), 64)
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def row_ln_emulate(x, gamma, beta, per, planted=None):
    """row_ln of csrc/text.hip / csrc/vision.hip in fp32 on the CPU (rsqrt and the division correctly rounded, nothing contracted).
    Planted error: the variance over 256 * PER columns instead of C."""
    rows, C = x.shape
    width = ROW_THREADS * per
    assert C <= width
    col = (torch.arange(ROW_THREADS)[None, :] + ROW_THREADS * torch.arange(per)[:, None])          # [PER][256]
    live = (col < C)
    xp = torch.cat([x.float(), torch.zeros(rows, width - C)], 1)[:, col]                             # [rows][PER][256]
    cf = torch.tensor(float(C), dtype=F32)
    mean = _block_sum(xp) / cf
    d = torch.where(live, xp - mean[:, None, None], torch.zeros(()))
    var = _block_sum(d * d) / (torch.tensor(float(width), dtype=F32) if planted == "variance_over_width" else cf)
    rstd = torch.rsqrt(var + torch.tensor(EPS, dtype=F32))
    y = (x.float() - mean[:, None]) * rstd[:, None] * gamma + beta
    return y


ROW_PLANTED = ("variance_over_width",)


def _row_table():
    cases = []
    for ci, C in enumerate(ROW_CS):
        for ki, kind in enumerate(ROW_KINDS):
            a, b = (ci + ki) % 3, (ci + 2 * ki + 1) % 3          # over the table: every (input, output) type pair, every kind with every type
            cases.append(Case(id="embed-C%d-%s" % (C, kind), op="text_embed", C=C, kind=kind, ydt=F16))
            cases.append(Case(id="final-C%d-%s-x%s-y%s" % (C, kind, DT_NAME[DTYPES[a]], DT_NAME[DTYPES[b]]), op="text_final", C=C, kind=kind,
                              xdt=DTYPES[a], ydt=DTYPES[b]))
            cases.append(Case(id="final_ext-C%d-%s-y%s" % (C, kind, DT_NAME[DTYPES[b]]), op="text_final_ext", C=C, kind=kind, xdt=F32, ydt=DTYPES[b]))
            cases.append(Case(id="vembed-C%d-%s-L%d" % (C, kind, (2, 5)[(ci + ki) % 2]), op="vision_embed", C=C, kind=kind, L=(2, 5)[(ci + ki) % 2],
                              ydt=F16))
            nulls = ("both", "pooled", "pooled32")[b]
            cases.append(Case(id="cls-C%d-%s-%s-%s" % (C, kind, DT_NAME[DTYPES[a]], nulls), op="vision_cls_ln", C=C, kind=kind, ydt=DTYPES[a],
                              outs=nulls))
        # y null: only the pooled row
        cases.append(Case(id="final-C%d-plain-pooled-only" % C, op="text_final", C=C, kind="plain", xdt=F32, ydt=DTYPES[ci % 3], y_null=True))
    return cases


ROWS = _row_table()
ROW_BY_ID = {c.id: c for c in ROWS}
ROW_N, ROW_L = 2, 3          # the text row cases: two prompts of three tokens


# ---------------------------------------------------------------------------------------------------------------------------
# pooled index (csrc/text.hip: pooled_index) and the id clamp
# ---------------------------------------------------------------------------------------------------------------------------
POOL_LS = (1, 63, 64, 65, 77, 128)
POOL_EOS = 7          # any id other than 2 takes the EOS rule


def pooled_index_ref(ids, eos, planted=None):
    """transformers' CLIPTextTransformer: eos == 2 -> the first position of the largest id; otherwise the first position holding eos, 0
    when there is none.  Planted errors: the last match; the EOS rule falling back to the argmax when there is no EOS."""
    ids = [int(v) for v in ids]
    L = len(ids)
    if eos == 2:
        m = max(ids)
        hits = [l for l in range(L) if ids[l] == m]
    else:
        hits = [l for l in range(L) if ids[l] == eos]
        if not hits:
            if planted == "eos_falls_back_to_argmax":
                m = max(ids)
                return [l for l in range(L) if ids[l] == m][0]
            return 0
    return hits[-1] if planted == "last_match" else hits[0]


POOL_PLANTED = ("last_match", "eos_falls_back_to_argmax")


def pool_table(L):
    """[(name, eos, ids [L], expected index)] of a length: every placement the length admits"""
    base = [10 + (l * 7) % 23 for l in range(L)]          # 10 .. 32, no 2 and no POOL_EOS
    rows = []

    def add(name, eos, marks, want):
        ids = list(base)
        for pos, val in marks:
            ids[pos] = val
        rows.append((name, eos, ids, want))

    big = 900
    add("argmax at 0", 2, [(0, big)], 0)
    add("argmax at L-1", 2, [(L - 1, big)], L - 1)
    if L > 64:
        add("argmax at 64", 2, [(64, big)], 64)
    if L > 70:
        add("argmax tie (5, 70)", 2, [(5, big), (70, big)], 5)
        add("argmax tie (6, 70), one lane", 2, [(6, big), (70, big)], 6)
    add("eos at 0", POOL_EOS, [(0, POOL_EOS)], 0)
    add("eos at L-1", POOL_EOS, [(L - 1, POOL_EOS)], L - 1)
    if L >= 63:
        add("eos twice, two lanes", POOL_EOS, [(9, POOL_EOS), (40, POOL_EOS)], 9)
    if L > 64:
        add("eos twice, one lane", POOL_EOS, [(L - 65, POOL_EOS), (L - 1, POOL_EOS)], L - 65)
    add("eos absent", POOL_EOS, [(L // 2, big)], 0)
    add("eos and a larger id elsewhere", POOL_EOS, [(L - 1, POOL_EOS), (0, big), (L // 2, big)], L - 1)
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# text_proj, text_store, vision_vt, vision_patchify, clip_resize_aa
# ---------------------------------------------------------------------------------------------------------------------------
PROJ = [Case(id="proj-C%d-P%d-N%d-%s" % (C, P, N, DT_NAME[dt]), C=C, P=P, N=N, dt=dt)
        for (C, P) in ((1, 1), (63, 5), (64, 4), (65, 7), (1280, 6)) for N in (1, 3) for dt in DTYPES]


def proj_problem(c):
    g = _gen("tproj", c.C, c.P)
    a, w = torch.randn(3, c.C, generator=g)[:c.N], torch.randn(c.P, c.C, generator=g) / math.sqrt(c.C)
    ref = a.double() @ w.double().t()
    bound = helpers.igemm_bound(ref, a.double().abs() @ w.double().abs().t(), c.C, 1.0, c.dt)
    return a, w, ref, bound


def proj_emulate(c):
    """text_proj_kernel: lanes over c in steps of 64 with an fma chain, then the wave butterfly"""
    a, w, _, _ = proj_problem(c)
    Cp = -(-c.C // 64) * 64
    ap = torch.cat([a, torch.zeros(c.N, Cp - c.C)], 1).reshape(c.N, 1, -1, 64)
    wp = torch.cat([w, torch.zeros(c.P, Cp - c.C)], 1).reshape(1, c.P, -1, 64)
    s = torch.zeros(c.N, c.P, 64)
    for i in range(Cp // 64):
        s = NF._fma(ap[:, :, i], wp[:, :, i], s)
    return NF._xor_tree(s, 64).to(c.dt)


STORE_NS = (1, 255, 257, 4096 * 256 + 17)          # op_text_store: at most 4096 workgroups of 256: the last takes a second trip

VT = [Case(id="vt-L%d-Lk%d-C%d-N%d-ld%s" % (L, Lk, C, N, "3C" if q else "C"), L=L, Lkpad=Lk, C=C, N=N, qkv=q)
      for (L, Lk) in ((1, 32), (31, 32), (32, 32), (33, 64), (33, 96), (257, 288)) for C in (32, 96) for N in (1, 2) for q in (False, True)]


def vt_expected(v, N, L, C, Lkpad, planted=None, after=None):
    """v [N*L][C] fp16 -> vt [N][C][Lkpad]; planted: rows >= L are copied too (`after`: what follows the last image's rows)"""
    out = torch.zeros(N, C, Lkpad, dtype=F16)
    rows = v if after is None else torch.cat([v, after], 0)
    for n in range(N):
        take = min(Lkpad, rows.shape[0] - n * L) if planted == "copies_rows_past_L" else L
        out[n, :, :take] = rows[n * L:n * L + take].t()
    return out


VT_PLANTED = ("copies_rows_past_L",)

PATCH = [Case(id="patch-S%d-p%d-K%d-%s" % (S, p, K, kind), S=S, p=p, Kpad=K, kind=kind)
         for (S, p, K) in ((14, 14, 640), (28, 14, 704), (6, 2, 64), (3, 1, 64)) for kind in ("f32_norm", "u8_norm", "f16_plain", "bf16_norm")]

RESIZE_SIZES = ((8, 8, 8, 8), (5, 7, 12, 9), (32, 48, 16, 24), (37, 53, 16, 24), (128, 66, 4, 3))
RESIZE_REFUSED = (134, 66, 4, 3)          # 134 / 4: sigma 16.25, 65 taps along y
RESIZE_MAX_TAPS = 63
RESIZE_TOL = 2e-6          # the project's tolerance on the [-1, 1] result (tests/test_gpu_vision_encoder.py)
RESIZE = []
for _i, _sz in enumerate(RESIZE_SIZES):
    for _j, _in in enumerate(("u8", "f32", "f16")):
        for _k, _out in enumerate(DTYPES):
            RESIZE.append(Case(id="resize-%dx%d-%dx%d-%s-%s%s" % (_sz + (_in, DT_NAME[_out], "-norm" if (_i + _j + _k) % 2 else "")),
                               size=_sz, src=_in, out=_out, norm=bool((_i + _j + _k) % 2)))


def resize_taps(n_in, n_out):
    """taps along one axis, restated from gauss_taps (csrc/vision.hip)"""
    sigma = max((n_in / n_out - 1.0) / 2.0, 0.001)
    k = int(max(2.0 * 2 * sigma, 3.0))
    return k + 1 if k % 2 == 0 else k


def resize_tol(ref, dt, std):
    """RESIZE_TOL on the [-1, 1] result is RESIZE_TOL / 2 on the [0, 1] one, / std_c after the normalisation; + one rounding of dt"""
    t = torch.full_like(ref, RESIZE_TOL * 0.5)
    if std is not None:
        t = t / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return t + store_round(ref, dt)
