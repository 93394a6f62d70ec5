"""The pure-data part of tests/test_gpu_norm_forms.py: the table of GroupNorm / LayerNorm cases (csrc/norm.hip) at their chunk, lane and
stride edges, their data, the fp64 reference with its element-wise bound, and a plain fp32 emulation of each kernel's arithmetic in the
kernel's own association that the host self-test (tests/test_norm_check_host.py) holds against the same bound.

The bound (every quantity from the fp64 reference, nothing from a GPU):

    |out - ref| <=   ulp16(ref)                                                        one fp16 quantum of the result (2^-24 below 2^-14)
                   + K * 2^-24 * (1 + log2 n) * (kappa * |gamma| * (1 + |xhat|) + |beta|) * slope   the statistics term

    n      the count the statistics run over (rows * channels per group; C for LayerNorm),
    kappa  GroupNorm: 1 + mean^2 / (var + eps) -- the kernels form the variance as E[x^2] - mean^2, whose rounding errors are relative to
           E[x^2], not to var; LayerNorm (two passes over registers, no cancellation): 1,
    xhat   (x - mean) * rstd, slope = 1.1 with SiLU (its largest derivative), else 1.

K is NOT derived: it is the smallest power of two for which the fp32 emulations below stay at or below 0.5 of the bound on every case of
the tables (measured against the fp64 reference; the factor 2 is the margin for rsqrtf, __expf, v_rcp_f32 and the contractions to fma the
emulation replaces by correctly rounded operations).  The rounding part alone already meets that criterion -- a round-to-nearest is off by
at most half a quantum -- so K is decided by the statistics alone.

    GN_K = 2^-1 (two-kernel and fused GroupNorm), LN_K = 2^-2 (LayerNorm)
    worst emulated |err| / bound: 0.500 for every family (an element that rounds at a tie spends half a quantum whatever the statistics
    do), 0.471 for the `offset` kind alone.  The figure that decides K is stat_part(): the share of the statistics term in use once that
    half quantum is taken off -- emulated 0.285 (two-kernel), 0.420 (two-kernel, offset), 0.442 (fused), 0.327 (fused, offset), 0.464
    (LayerNorm); one power of two less and it passes 0.5.  Printed by tests/test_norm_check_host.py::
    test_emulation_stays_within_half_the_bound; the figures measured on the GPU are in DESIGN.md section 6.

Data kinds: `plain` (mean 0.5, std 1, a per-channel component so that neighbouring channels differ), `spike` (plain plus one value of
about 64 sigma in the last row of every row block of the statistics launch and in the last row of the image, each in another group: every
tail row decides the statistics of its group), `offset` (fp32 only: group mean = 32 x its std, the cancellation regime of E[x^2] - mean^2),
`flat` (one group of the last image constant: var = 0, the clamp, rstd = 1 / sqrt(eps)).
"""
import functools
import math
import types
import zlib

import torch

F16, F32 = torch.float16, torch.float32
EPS = 1e-5
U = 2.0 ** -24
GN_K = 2.0 ** -1
LN_K = 2.0 ** -2
GN_STATS_BLOCKS, GN_APPLY_BLOCKS = 768, 2048       # csrc/ops.h: kGnStatsBlocks, kGnApplyBlocks
FUSED_RL, FUSED_CH, FUSED_BYTES = 102, 80, 512 * 1024   # csrc/norm.hip: kGnFusedRL, kGnFusedCh, kGnFusedBytes


class Case(dict):
    __getattr__ = dict.get

    def __hash__(self):
        return hash(self["name"])

    def __eq__(self, other):
        return self is other


def mirror_launch_shape(imgs, rows, C, which):
    """gn_rows_per_block of csrc/norm.hip restated: (rows_per_block, chunks) of the statistics (which = 0) / apply (1) launch; the host
    test holds every declared value against ctrl_gn_launch_shape"""
    rpi = 256 // (C // 8)
    target = (GN_STATS_BLOCKS, GN_APPLY_BLOCKS)[which]
    chunks = -(-target // imgs)
    rpb = max(-(-rows // chunks), 8 * rpi)
    rpb = -(-rpb // rpi) * rpi
    return rpb, -(-rows // rpb)


# ------------------------------------------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------------------------------------------
GN = []          # two-kernel GroupNorm: gn_stats_kernel<T> + gn_apply_kernel<T>
LAYOUTS = ("wide_in", "wide_out", "split", "padded0", "padded3", "sharded")


def gn(name, imgs, rows, C, G=32, dt="f16", kind="plain", silu=False, layout=None, halves=False, stats=None, apply=None):
    """stats / apply: the DECLARED (rows_per_block, chunks) of the two launches (None: the mirror's); halves: x is one half of rows 2 C wide
    (ldx = 2 C) and the case runs both halves, each with its half of gamma and beta"""
    c = Case(name="%s %s %s%s" % (name, dt, kind, " silu" if silu else ""), imgs=imgs, rows=rows, C=C, G=G, dt=dt, kind=kind, silu=silu,
             layout=layout, halves=halves, stats=stats or mirror_launch_shape(imgs, rows, C, 0),
             apply=apply or mirror_launch_shape(imgs, rows, C, 1))
    GN.append(c)
    return c


# lane geometry: rpi = 256 / (C / 8) rows per iteration; idle threads at C = 320, 640, 960, 1280; cg = 10 straddles a lane's 8 channels
GEOMETRIES = [("C8 G1", 8, 1, False), ("C8 G2", 8, 2, False), ("C8 G8", 8, 8, False), ("C320", 320, 32, False), ("C640", 640, 32, False),
              ("C960", 960, 32, False), ("C1280", 1280, 32, False), ("C2048", 2048, 32, False), ("halves C1280 G16", 1280, 16, True),
              ("halves C64 G16", 64, 16, True)]
for _nm, _C, _G, _hv in GEOMETRIES:
    _rpi = 256 // (_C // 8)
    _rows = 2 * 8 * _rpi + 3 if _rpi < 256 else 300          # two full row blocks and a 3-row one (C = 8: 300 rows, one block)
    for _dt in ("f16", "f32"):
        gn("geometry %s rows%d" % (_nm, _rows), 2, _rows, _C, _G, _dt, "spike", halves=_hv)
    gn("geometry %s rows%d" % (_nm, _rows), 2, _rows, _C, _G, "f16", "plain", silu=True, halves=_hv)
    gn("geometry %s rows%d" % (_nm, _rows), 2, _rows, _C, _G, "f32", "offset", halves=_hv)
    gn("geometry %s rows%d" % (_nm, _rows), 2, _rows, _C, _G, "f32" if _C % 16 else "f16", "flat", silu=True, halves=_hv)

# rows at ONE chunk: 1, rpi - 1, rpi + 1, 8 rpi - 1, 8 rpi
for _dt in ("f16", "f32"):
    for _rows in (1, 7, 255, 257, 2047, 2048):
        gn("one chunk C8 G2 rows%d" % _rows, 2, _rows, 8, 2, _dt, "spike", stats=(2048, 1), apply=(2048, 1))
    for _rows in (1, 5, 7, 47, 48):
        gn("one chunk C320 rows%d" % _rows, 1, _rows, 320, 32, _dt, "spike", stats=(48, 1), apply=(48, 1))

# chunk counts of the statistics launch: 2, 3, 5 (empty and ragged quarters of the last workgroup's reduction), 8, 13, 14, 34, 40 (the 8-wide
# load block plus a tail: 34 -> quarters of 9, 9, 9, 7; 40 -> 10 each)
for _dt in ("f16", "f32"):
    gn("2 chunks, the second one row", 1, 49, 320, 32, _dt, "spike", stats=(48, 2))
    gn("3 chunks", 1, 20, 1280, 32, _dt, "spike", stats=(8, 3))
    gn("5 chunks", 1, 37, 1280, 32, _dt, "spike", stats=(8, 5))
    gn("8 chunks", 2, 63, 1280, 32, _dt, "spike", stats=(8, 8))
    gn("13 chunks", 1, 100, 2048, 32, _dt, "spike", stats=(8, 13))
    gn("14 chunks", 2, 333, 640, 32, _dt, "spike", stats=(24, 14))
    gn("34 chunks", 1, 1589, 320, 32, _dt, "spike", stats=(48, 34))
    gn("40 chunks", 1, 320, 2048, 32, _dt, "spike", stats=(8, 40))
    # rows = 1 .. 7 (mod 8 rpi) at rpi = 1: the last block runs the unrolled loop, then the tail (fp32 statistics: 4 loads; apply: 4)
    for _r in range(9, 16):
        gn("tail rows%d C1280" % _r, 1, _r, 1280, 32, _dt, "spike", stats=(8, 2), apply=(8, 2))

# the one large case: the smallest shape that leaves the 8 rpi floor (statistics: 11 rows per block = one unrolled pass + a 3-row tail)
gn("large 8 x 1056 x 1280", 8, 1056, 1280, 32, "f16", "spike", stats=(11, 96), apply=(8, 132))

# layouts, on three geometries
for _nm, _C, _G, _hv, _rows in (("C320", 320, 32, False, 49), ("C1280", 1280, 32, False, 20), ("halves C1280 G16", 1280, 16, True, 20)):
    for _lay in LAYOUTS:
        for _dt in ("f16", "f32"):
            gn("layout %s %s rows%d" % (_lay, _nm, _rows), 2, _rows, _C, _G, _dt, "spike", silu=(_lay in ("split", "sharded")), layout=_lay,
               halves=_hv)

GN_CHUNK_COUNTS = (1, 2, 3, 5, 8, 13, 14, 34, 40, 96)         # every one of them has to appear among the statistics launches of GN


def fused_max_rows(dt):
    return FUSED_BYTES // (FUSED_CH * (4 if dt == "f32" else 2))


FUSED = []       # gn_fused_kernel<T>: 102 row lanes, 4 loads in flight: rows around 102 and 4 * 102, and the largest map it takes
for _C in (320, 640, 1280, 2560):
    for _dt in ("f16", "f32"):
        for _rows in (1, 101, 102, 103, 407, 408, 409):
            _kind, _silu = (("spike", False) if _rows in (101, 103, 407, 409) else ("plain", True))
            FUSED.append(Case(name="fused C%d rows%d %s %s" % (_C, _rows, _dt, _kind), imgs=2, rows=_rows, C=_C, G=32, dt=_dt, kind=_kind,
                              silu=_silu, fused=True))
for _dt in ("f16", "f32"):
    FUSED.append(Case(name="fused C320 largest rows%d %s spike" % (fused_max_rows(_dt), _dt), imgs=1, rows=fused_max_rows(_dt), C=320, G=32,
                      dt=_dt, kind="spike", silu=False, fused=True))
FUSED.append(Case(name="fused C1280 rows409 f32 offset", imgs=2, rows=409, C=1280, G=32, dt="f32", kind="offset", silu=False, fused=True))
FUSED.append(Case(name="fused C640 rows103 f16 flat", imgs=2, rows=103, C=640, G=32, dt="f16", kind="flat", silu=True, fused=True))

LN_C = (8, 320, 504, 512, 520, 1024, 1032, 1280, 2048)        # NCH = 1 up to 512, 2 up to 1024, else 4: both sides of both boundaries
LN_M = (1, 3, 4, 5, 33)                                        # four rows per workgroup
LN = []          # layernorm_kernel<NCH, T>; M = 33 runs dense, every other M inside wider rows (ldx = C + 16, ldy = C + 24)
for _C in LN_C:
    for _M in LN_M:
        for _dt in ("f16", "f32"):
            LN.append(Case(name="ln C%d M%d %s%s" % (_C, _M, _dt, "" if _M == 33 else " wide"), C=_C, M=_M, dt=_dt, wide=_M != 33))
LN_ADD = []      # op_layernorm_add: xsum = x + addv[(row / rows_per_img) % vmod], y = LayerNorm(xsum); M = 33 is no multiple of 21 or 10
for _C in (320, 520, 1032):
    for _rpi, _vmod in ((1, 1), (7, 3), (5, 2)):
        for _dt in ("f16", "f32"):
            LN_ADD.append(Case(name="ln_add C%d rpi%d vmod%d %s" % (_C, _rpi, _vmod, _dt), C=_C, M=33, dt=_dt, wide=True, add=True,
                               rows_per_img=_rpi, vmod=_vmod))


def ln_nch(C):
    return 1 if C <= 512 else (2 if C <= 1024 else 4)


def kernel_of(c):
    """the template instance a case runs (the completeness test wants every one of them in the tables)"""
    T = "float" if c.dt == "f32" else "half_t"
    if c.fused:
        return ("gn_fused_kernel<%s>" % T,)
    if c.M is not None:
        return ("layernorm_kernel<%d, %s>" % (ln_nch(c.C), T),)
    return ("gn_stats_kernel<%s>" % T, "gn_apply_kernel<%s>" % T)


KERNELS = tuple(k % T for k in ("gn_stats_kernel<%s>", "gn_apply_kernel<%s>", "gn_fused_kernel<%s>") for T in ("half_t", "float")) + tuple(
    "layernorm_kernel<%d, %s>" % (n, T) for n in (1, 2, 4) for T in ("half_t", "float"))


# ------------------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _round(t, dt):
    return t.half().float() if dt == "f16" else t.float()


def spike_rows(rows, rpb):
    """last row of every row block of the statistics launch (the last block's is the last row of the image)"""
    return sorted({min(rows, (k + 1) * rpb) - 1 for k in range(-(-rows // rpb))})


def fused_spike_rows(rows):
    """last row of the image and the last rows of the first and fourth pass over the 102 row lanes"""
    return sorted({r for r in (101, 407, rows - 1) if r < rows})


@functools.lru_cache(maxsize=4)
def gn_data(c):
    """x [imgs][rows][Ct] (Ct = 2 C for the halves form, fp32 CPU, fp16-representable for fp16 input), gamma, beta [Ct], and the
    (image, row, channel) of every spike"""
    Ct = c.C * (2 if c.halves else 1)
    Gt = c.G * (2 if c.halves else 1)
    cg = c.C // c.G
    g = _gen("gn", c.imgs, c.rows, Ct, Gt, c.dt, c.kind, c.seed)
    chan = torch.randn(Ct, generator=g)
    x = 0.5 + 0.9 * torch.randn(c.imgs, c.rows, Ct, generator=g) + 0.45 * chan
    spikes = []
    if c.kind == "offset":
        x = x - 0.5 + 32.0 * math.sqrt(0.81 + 0.2025)
    elif c.kind == "flat":
        x[c.imgs - 1, :, (Gt - 1) * cg:] = 1.5
    elif c.kind == "spike":
        rs = fused_spike_rows(c.rows) if c.fused else spike_rows(c.rows, c.stats[0])
        k = 0
        for i in range(c.imgs):
            for r in rs:
                for h in range(2 if c.halves else 1):
                    ch = h * c.C + (k % c.G) * cg + (7 * k) % cg
                    x[i, r, ch] = 64.0 if k % 2 == 0 else -63.0
                    spikes.append((i, r, ch))
                k += 1
    gamma = (1.0 + 0.3 * torch.randn(Ct, generator=g)).float()
    beta = (0.2 * torch.randn(Ct, generator=g)).float()
    return types.SimpleNamespace(x=_round(x, c.dt), gamma=gamma, beta=beta, spikes=spikes)


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 reference and bound
# ------------------------------------------------------------------------------------------------------------------------------------
def ulp16(ref):
    """the fp16 quantum at |ref|: 2^(e - 10) for 2^e <= |ref| < 2^(e + 1), 2^-24 below 2^-14"""
    _, e = torch.frexp(ref.abs().double().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 11)


def stat_part(err, ref, bound):
    """how much of the STATISTICS term an error uses once the half quantum a correct rounding may cost is taken off: the total |err| / bound
    sits at 0.5 whenever one element rounds at a tie, whatever the statistics do; this figure is the one that moves with them"""
    q = ulp16(ref)
    return float(((err - 0.5 * q) / (bound - q)).max().clamp_min(0.0))


def silu64(t):
    return t * torch.sigmoid(t)


def gn_sums(x, G):
    """x [imgs][rows][C] fp64 -> (sum, sum of squares) per (image, group), [imgs][G]"""
    imgs, rows, C = x.shape
    xg = x.reshape(imgs, rows, G, C // G)
    return xg.sum((1, 3)), (xg * xg).sum((1, 3))


def gn_out(x, s, ss, n, gamma, beta, G, silu, eps=EPS, K=GN_K):
    """fp64 GroupNorm of x [imgs][rows][C] from the group sums s, ss [imgs][G] over n elements -> (result, bound)"""
    imgs, rows, C = x.shape
    cg = C // G
    mean = s / n
    var = (ss / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    ex = lambda t: t.repeat_interleave(cg, 1)[:, None, :]
    xhat = (x - ex(mean)) * ex(rstd)
    ref = xhat * gamma.double() + beta.double()
    if silu:
        ref = silu64(ref)
    kappa = ex(1.0 + mean * mean / (var + eps))
    stat = K * U * (1.0 + math.log2(n)) * (kappa * gamma.double().abs() * (1.0 + xhat.abs()) + beta.double().abs()) * (1.1 if silu else 1.0)
    return ref, ulp16(ref) + stat


def gn_reference(x, gamma, beta, G, silu):
    x = x.double()
    s, ss = gn_sums(x, G)
    return gn_out(x, s, ss, x.shape[1] * (x.shape[2] // G), gamma, beta, G, silu)


def halves_of(c):
    """column ranges a case runs: [(col0, C)]"""
    return [(h * c.C, c.C) for h in range(2 if c.halves else 1)]


@functools.lru_cache(maxsize=4)
def gn_problem(c):
    """data + per half (col0, ref, bound); shared by the tests of a case and never modified"""
    D = gn_data(c)
    D.refs = []
    for col0, C in halves_of(c):
        ref, bound = gn_reference(D.x[:, :, col0:col0 + C], D.gamma[col0:col0 + C], D.beta[col0:col0 + C], c.G, c.silu)
        D.refs.append((col0, ref, bound))
    return D


def ln_reference(x, gamma, beta, eps=EPS, K=LN_K, count=None):
    """fp64 LayerNorm over the last dim of x [M][C] -> (result, bound)"""
    x = x.double()
    C = count or x.shape[1]
    mean = x.sum(1, keepdim=True) / C
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / C if count is None else ((x * x).sum(1, keepdim=True) / C - mean * mean)
    xhat = d / torch.sqrt(var + eps)
    ref = xhat * gamma.double() + beta.double()
    stat = K * U * (1.0 + math.log2(x.shape[1])) * (gamma.double().abs() * (1.0 + xhat.abs()) + beta.double().abs())
    return ref, ulp16(ref) + stat


def ln_vec_index(M, rows_per_img, vmod):
    return (torch.arange(M) // rows_per_img) % vmod


@functools.lru_cache(maxsize=8)
def ln_problem(c):
    """x [M][C], gamma, beta; with `add`: addv [vmod][C] and xsum = the sum as the kernel stores it (fp16 input: rounded ONCE to fp16, and
    that is what is normalised); ref, bound of LayerNorm(xsum or x)"""
    g = _gen("ln", c.C, c.M, c.dt, bool(c.add), c.rows_per_img, c.vmod, c.seed)
    chan = torch.randn(c.C, generator=g)
    x = _round(0.5 + 0.9 * torch.randn(c.M, c.C, generator=g) + 0.45 * chan, c.dt)
    P = types.SimpleNamespace(x=x, gamma=(1.0 + 0.3 * torch.randn(c.C, generator=g)).float(), beta=(0.2 * torch.randn(c.C, generator=g)).float(),
                              addv=None, xsum=None)
    src = x
    if c.add:
        P.addv = torch.randn(c.vmod, c.C, generator=g).float()
        P.xsum = _round(x + P.addv[ln_vec_index(c.M, c.rows_per_img, c.vmod)], c.dt)       # one fp32 add (exact in fp32 terms), one rounding
        src = P.xsum
    P.ref, P.bound = ln_reference(src, P.gamma, P.beta)
    return P


# ------------------------------------------------------------------------------------------------------------------------------------
# plain fp32 emulations of the kernels' arithmetic, each in the kernel's own association
# ------------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _xor_tree(a, width):
    """a [..., width] -> the butterfly `for o = width / 2 .. 1: a += shfl_xor(a, o)`; every lane ends with the same value"""
    idx = torch.arange(width)
    o = width // 2
    while o >= 1:
        a = a + a[..., idx ^ o]
        o //= 2
    return a[..., 0]


def _seq_sum(t, dim):
    """sequential fp32 sum along `dim`, in index order"""
    acc = torch.zeros_like(t.select(dim, 0))
    for k in range(t.shape[dim]):
        acc = acc + t.select(dim, k)
    return acc


def _pad(t, dim, size):
    if t.shape[dim] == size:
        return t
    shape = list(t.shape)
    shape[dim] = size - t.shape[dim]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim)          # (adding +0 changes no fp32 sum)


def emulate_gn_sums(x, G, rpi, rpb, parts):
    """x [imgs][rows][C] fp32 -> (s, ss) [imgs][G] fp32 as gn_stats_kernel (rpi = 256 / (C / 8), parts = 8) or the statistics half of
    gn_fused_kernel (rpi = 102 row lanes, one block, parts = 16) add them: per-lane partials over the lane's rows in row order (sum of
    squares by fma), per-workgroup sums of a group by `parts` lanes striding its rpi * cg LDS slots and a xor tree, then the chunks of an
    image in four quarters (index order inside, quarter order outside)"""
    x = x.float()
    imgs, rows, C = x.shape
    cg = C // G
    chunks = -(-rows // rpb)
    xr = _pad(x, 1, chunks * rpb).reshape(imgs, chunks, rpb // rpi, rpi, C)
    s = torch.zeros(imgs, chunks, rpi, C)
    ss = torch.zeros(imgs, chunks, rpi, C)
    for k in range(rpb // rpi):
        f = xr[:, :, k]
        s = s + f
        ss = _fma(f, f, ss)
    n = cg * rpi
    e = torch.arange(n)
    idx = ((e // cg) * C + e % cg)[None, :] + (torch.arange(G) * cg)[:, None]          # [G][n]: LDS slot of element e of group g
    npad = -(-n // parts) * parts

    def block_sum(t):
        gs = _pad(t.reshape(imgs, chunks, rpi * C)[:, :, idx], 3, npad).reshape(imgs, chunks, G, npad // parts, parts)
        return _xor_tree(_seq_sum(gs, 3), parts)                                        # [imgs][chunks][G]

    ps, pss = block_sum(s), block_sum(ss)
    if chunks == 1:
        return ps[:, 0], pss[:, 0]
    cq = (chunks + 3) // 4

    def quarters(t):
        q = _seq_sum(_pad(t, 1, 4 * cq).reshape(imgs, 4, cq, G), 2)
        return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]

    return quarters(ps), quarters(pss)


def emulate_gn_apply(x, s, ss, stat_rows, gamma, beta, G, silu, eps=EPS):
    """gn_apply_kernel / the apply half of gn_fused_kernel in fp32: (scale, shift) per channel, y = fp16(x * scale + shift) (SiLU)"""
    x = x.float()
    imgs, rows, C = x.shape
    cg = C // G
    inv_cnt = torch.tensor(1.0, dtype=F32) / (torch.tensor(float(stat_rows), dtype=F32) * torch.tensor(float(cg), dtype=F32))
    mean = s * inv_cnt
    var = (ss * inv_cnt - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    ex = lambda t: t.repeat_interleave(cg, 1)[:, None, :]
    sc = ex(rstd) * gamma
    sf = beta - ex(mean) * sc
    f = x * sc + sf
    if silu:
        f = f * (1.0 / (1.0 + torch.exp(-f)))
    return f.half()


def emulate_gn(c, x, gamma, beta):
    """one half of a two-kernel or fused case through the emulation -> fp16 [imgs][rows][C]"""
    imgs, rows, C = x.shape
    if c.fused:
        s, ss = emulate_gn_sums(x, c.G, FUSED_RL, -(-rows // FUSED_RL) * FUSED_RL, 16)
        return emulate_gn_apply(x, s, ss, rows, gamma, beta, c.G, c.silu)
    rpi = 256 // (C // 8)
    if c.layout == "sharded":
        ra = shard_rows(rows)
        parts = [x[:, :ra], x[:, ra:]]
        sums = [emulate_gn_sums(p, c.G, rpi, mirror_launch_shape(imgs, p.shape[1], C, 0)[0], 8) for p in parts]
        s, ss = sums[0][0] + sums[1][0], sums[0][1] + sums[1][1]
        return torch.cat([emulate_gn_apply(p, s, ss, rows, gamma, beta, c.G, c.silu) for p in parts], 1)
    s, ss = emulate_gn_sums(x, c.G, rpi, c.stats[0], 8)
    return emulate_gn_apply(x, s, ss, rows, gamma, beta, c.G, c.silu)


def shard_rows(rows):
    """rows of the first of the two row shards of an image (`sharded` layout); uneven on purpose"""
    return rows // 2 + 1


def emulate_ln(x, gamma, beta, eps=EPS):
    """layernorm_kernel in fp32: lane l of the row's wavefront holds channels (l + 64 i) * 8 .. + 8, sums them in (i, j) order, wave xor
    tree, mean, then the squared deviations the same way (fma), rstd, y = fp16(((v - mean) * rstd) * gamma + beta)"""
    x = x.float()
    M, C = x.shape
    nch = ln_nch(C)
    v = _pad(x, 1, nch * 512).reshape(M, nch, 64, 8)
    live = (_pad(torch.ones(1, C), 1, nch * 512).reshape(1, nch, 64, 8) > 0)
    s = torch.zeros(M, 64)
    for i in range(nch):
        for j in range(8):
            s = s + v[:, i, :, j]
    Cf = torch.tensor(float(C), dtype=F32)
    mean = (_xor_tree(s, 64) / Cf)[:, None]
    q = torch.zeros(M, 64)
    for i in range(nch):
        for j in range(8):
            d = torch.where(live[:, i, :, j], v[:, i, :, j] - mean, torch.zeros(()))
            q = _fma(d, d, q)
    rstd = torch.rsqrt(_xor_tree(q, 64) / Cf + torch.tensor(eps, dtype=F32))[:, None]
    return (((x - mean) * rstd) * gamma + beta).half()
