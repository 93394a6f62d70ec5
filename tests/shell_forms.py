"""The per-pixel "shell" kernels around the KL-VAE and the three backbone UNets (vae_posterior, vae_dec_head, vae_dec_tail<COUT>,
vae_time_conv<OC, VEC> of csrc/vae.hip; unet_skip_join, i2v_latent_encoder, adaptive_avgpool_nhwc, unet_text_time of csrc/unet.hip) at
their tile, frame and lane edges: case tables, problem builders seeded by case id, fp64 references with element-wise bounds or exact
restatements, fp32 emulations in the kernels' own association and the planted errors the checks have to reject.  Pure data: imports no
GPU code.

    GPU tests: tests/test_gpu_shell_forms.py        host self-test (no GPU): tests/test_shell_check_host.py

u = 2^-24 (half an fp32 ulp, relative); out_quantum(ref, dt) one quantum of the output type at |ref| (0 for fp32, where the fp32 value
itself is what the bound speaks of).  An fma chain of K terms started at a bias costs (K + 1) u mag in any order, mag = |bias| + sum of
the |products| (helpers.igemm_bound's argument); every further rounded operation on the value adds one u of what it works on.

skip_join.  v = skip + res: ONE fp32 add (an addition cannot be contracted), hi = fp16(v), lo = fp16(v - float(hi)) (the difference is
    exact in fp32): restated in torch and compared bit for bit, the whole mirror row with its poison (between hi and lo, behind lo).
vae_posterior.  q = bq + wq x: 2 lat fmas from the bias, (2 lat + 2) u mag on mean and on the logvar before its clamp (the clamp is
    1-Lipschitz and continuous: no element is exempt); without wq the moments are x itself, exact.  std = expf(0.5 lv), var = expf(lv):
    ref (k d_lv + PO_E u (1 + |k lv|)), k = 0.5 | 1 (the product 0.5 lv is exact; the argument's rounding and expf's own ulps are PO_E).
    mode = mean s: d_mean |s| + u |ref|; sample = fma(std, eps, mean) s: (d_std |eps| + d_mean + u |std eps + mean|) |s| + u |ref|;
    every result + one output quantum.  fp16 MOMENTS: exp(20) overflows: where |ref| >= 65520 the output must be that infinity.
vae_dec_head.  v = z s (one rounding), q = bpq + wpq v (lat fmas), out = b + sum over the taps INSIDE the map of w q (9 lat fmas):
    (9 lat + lat + 4) u mag, mag = |z| |s| |wpq| |w| + |bpq| |w| + |b| (the fp64 composition of the two convolutions over absolute
    values).  Element-wise, so a single border pixel that saw bpq outside the map shows.
vae_dec_tail.  The statistics are given (fp32 roundings of the fp64 group sums).  The activated map: norm_forms.gn_out's statistics
    term (GN_K u (1 + log2 n) (kappa |gamma| (1 + |xhat|) + |beta|), without its fp16 quantum -- the map stays fp32) carried through
    SiLU's slope 1.1, + silu_f's own error (helper_forms._equick: tower_forms' e_quick at k = 1); that through sum |w| over the 9 C
    taps (zero outside the map: the convolution pads the ACTIVATED map), + (9 C + 2) u mag, mag = |act| * |w| + |b|.  Every other kind
    and dtype follows bit for bit from the kernel's own fp32 SAMPLE: one rounding to the module dtype, v / 2 + 0.5 (one rounding,
    contracted or not: v / 2 is exact) clamped, one product by 255, round half to even, NHWC bytes.
vae_time_conv.  acc = b + 3 OC fmas: (3 OC + 2) u mag, mag = |b| + |w| * |x| over the three frames (zero outside [0, F)); every other
    kind and dtype bit for bit from the fp32 SAMPLE as above.  The scalar kernel is the vector one's arithmetic per pixel: same bits.
i2v_latent_encoder.  Columns 0..3, keep and the precomputed pass are copies (bit for bit).  Columns 4..7, per token, from the fp64
    restatement's own intermediates; K = EN_K stands for the LayerNorm's rsqrt and subtraction, expf and erff:
      LayerNorm   dd_i = K u (mean|x| + |x_i|); rho = sum |d_j| dd_j / (4 (var + eps)) + K u; dxn = (dd rstd + |d| rstd rho) |g| + K u |xn|
      q, k, v     |W| dxn + 5 u |W| |xn|                                  (4 fmas from 0)
      scores      ds_j = 0.5 (|q| dk_j + dq |k_j|) + 5 u 0.5 |q| |k_j|     (4 products, 3 sums; the factor 0.5 is exact)
      weights     dw_j = w_j (ds_j + sum_i w_i ds_i + K u (1 + |s_j - m|) + (F + 2) u)
      o           sum_j (dw_j |v_j| + w_j dv_j) + (F + 2) u sum_j w_j |v_j|   (F fmas and the division)
      x1          |Wo| do + 11 u (|Wo| |o| + |bo| + |x|)
      hidden      da = |W1| dx1 + 6 u (|W1| |x1| + |b1|);  dh = 1.13 da + K u (|a| + da)     (1.13: the erf GELU's largest slope)
      out         |W2| dh + 19 u (|W2| |h| + |b2| + |x1|) + dx1
adaptive_avgpool.  The window's k values summed in fp32 row by row and divided once: (k + 1) u max|x| as the older test has it, + one
    output quantum; a one-element window (replication, identity) is exact: y = the conversion of x.
unet_text_time.  Text columns: the conversion to fp32, exact.  Sinusoids: helper_forms' sincos bound with its SC_C, SC_K unchanged
    (the kernel uses sincos_kernel's expressions), on time ids drawn from helper_forms.SC_TS.

Calibrated constants (helper_forms' rule: the smallest power of two for which the fp32 CPU emulation, in the kernel's association, stays
at or below 0.5 of the bound on this table, against the fp64 reference; the factor 2 is the margin for the device's expf, erff and
rsqrtf differing from the host's, which nobody has measured here).  Printed by tests/test_shell_check_host.py::
test_emulations_stay_within_their_bounds:
    PO_E = 2^1     share 0.50 on std and var (MOMENTS in fp32) of every case; 2^0 gives 1.00
    EN_K = 2^2     shares 0.22 (LayerNorm), 0.27 (softmax weights), 0.44 (erf GELU), each stage alone on the whole table
                   (enc_stage_shares); 2^1 gives 0.44, 0.48, 0.87.  The whole chain's emulation uses 0.004 of its bound: the derived
                   fma-chain terms take every product at its absolute value through five layers and hold most of it.
"""
import functools
import math

import torch
import torch.nn.functional as Fn

import helpers
import helper_forms as HF
import norm_forms as NF
import tower_forms as TF

U = 2.0 ** -24
F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8
DTYPES = (F32, F16, BF16)
DT_NAME = TF.DT_NAME
POISON = helpers._POISON
TINY = 2.0 ** -149
FP16_OVF = 65520.0          # the smallest magnitude that rounds to an fp16 infinity

# restated from the .hip files
THREADS = 256               # vae_posterior, vae_dec_head, vae_time_conv: one item per thread, 256 per workgroup
MAX_LAT = 8                 # kMaxLat
GROUP16 = 16                # vae_dec_head_kernel (and vae_conv_in_kernel): 16 output channels per thread
TAIL_W, TAIL_H, TAIL_CK = 32, 8, 32          # kTailW, kTailH, kTailCk
TC_FRAMES, TC_PV = 4, 4     # kTcFrames; PV of the vector kernel
JOIN_C, JOIN_P, JOIN_CPT = 32, 64, 8         # unet_skip_join_kernel: 32 c x 64 p per workgroup, 8 channels per thread
ENC_WTS = 288               # kI2vEncWts
SAMPLE, UNIT, BYTES = 0, 1, 2                # CTRL_VAE_DEC_SAMPLE / _UNIT / _U8
MODE, PSAMPLE, MOMENTS = 0, 1, 2             # CTRL_VAE_MODE / _SAMPLE / _MOMENTS

PO_E, EN_K = 2.0 ** 1, 2.0 ** 2

Case = TF.Case
quantum = TF.quantum
out_quantum = HF.out_quantum
check = HF.check
bits_equal = HF.bits_equal
pick = HF.pick
_gen = HF._gen
_fma = NF._fma


def enc_P(F):
    """pixels per workgroup of i2v_latent_encoder_kernel"""
    return THREADS // F


def _f32(v):
    return torch.tensor(v, dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------------
# the output epilogue shared by vae_dec_tail and vae_time_conv, restated bit for bit from the fp32 SAMPLE
# ---------------------------------------------------------------------------------------------------------------------------
def epilogue(s32, kind, dt, planted=None):
    """s32 fp32 [N][C][...] (the kernel's fp32 SAMPLE) -> what `kind` stores for the module dtype dt: SAMPLE in dt, UNIT fp32, BYTES uint8
    channels-last.  planted: half_away (round half away from zero), unit_unrounded (v not rounded to dt first), bytes_reversed (the four
    bytes of every 32-bit word of the channels-last result in the opposite order)"""
    if kind == SAMPLE:
        return s32.to(dt)
    v = s32 if planted == "unit_unrounded" else s32.to(dt).float()
    u = (v * _f32(0.5) + _f32(0.5)).clamp(0.0, 1.0)
    if kind == UNIT:
        return u
    p = u * _f32(255.0)
    r = torch.floor(p + _f32(0.5)) if planted == "half_away" else torch.round(p)
    q = r.to(U8).movedim(1, -1).contiguous()
    if planted == "bytes_reversed":
        q = q.reshape(-1, 4).flip(1).reshape(q.shape)
    return q


# ---------------------------------------------------------------------------------------------------------------------------
# unet_skip_join
# ---------------------------------------------------------------------------------------------------------------------------
JOIN_HWS, JOIN_C2S, JOIN_BFS, JOIN_COLS = (1, 63, 64, 65, 130), (32, 96), ((1, 1), (2, 3)), (0, 64)
JOIN_RES = (("none", F32),) + tuple((l, d) for l in ("4d", "5d") for d in DTYPES)
JOIN_MIRRORS = ("none", "plain", "split")
JOIN_GAP = 8          # a split mirror's lo half this many columns behind the tightest place


def _join_case(HW, C2, B, F, res, rdt, col, mirror, gap, wide, inplace=False):
    ld_out = col + C2 + 16
    lo_off = (col + C2 + gap) if mirror == "split" else 0
    return Case(id="join-HW%d-C%d-B%dF%d-%s%s-col%d-%s%s%s%s" % (HW, C2, B, F, res, "" if res == "none" else "-" + DT_NAME[rdt], col, mirror,
                                                               "-gap" if gap else "", "-wide" if wide else "", "-inplace" if inplace else ""),
                HW=HW, C2=C2, B=B, F=F, res=res, res_dt=rdt, col=col, mirror=mirror, lo_off=lo_off, ld_out=ld_out,
                ld_skip=ld_out if inplace else C2 + (8 if wide else 0), inplace=inplace)


JOIN = []
for _i, (_HW, _C2, (_B, _F)) in enumerate((p, c, bf) for p in JOIN_HWS for c in JOIN_C2S for bf in JOIN_BFS):
    _res, _rdt = JOIN_RES[_i % 7]
    _mir = JOIN_MIRRORS[_i % 3]
    JOIN.append(_join_case(_HW, _C2, _B, _F, _res, _rdt, JOIN_COLS[(_i // 2) % 2], _mir, JOIN_GAP if (_i // 3) % 2 else 0, bool((_i // 5) % 2)))
# the mid residual: added in place over the stream (skip is out32, col 0), with both mirrors
JOIN.append(_join_case(65, 96, 2, 3, "4d", F16, 0, "plain", 0, False, inplace=True))
JOIN.append(_join_case(65, 96, 2, 3, "5d", BF16, 0, "split", JOIN_GAP, False, inplace=True))
JOIN.append(_join_case(130, 32, 2, 3, "5d", F32, 64, "split", 0, True))
JOIN_BY_ID = {c.id: c for c in JOIN}


@functools.lru_cache(maxsize=None)
def join_problem(case_id):
    """skip fp32 [rows][C2] (some columns 2^-7 smaller: the lo halves of their values are fp16 subnormals; a few values near 3e4), res in
    the case's layout and dtype or None"""
    c = JOIN_BY_ID[case_id]
    g = _gen("join", case_id)
    rows = c.B * c.F * c.HW
    skip = torch.randn(rows, c.C2, generator=g) * 3.0
    skip[:, ::5] *= 2.0 ** -7
    skip[::7, 1] = 3.0e4
    res = None
    if c.res != "none":
        r4 = (torch.randn(c.B * c.F, c.C2, c.HW, generator=g) * 0.7).to(c.res_dt)          # (b f) c p
        res = r4 if c.res == "4d" else r4.reshape(c.B, c.F, c.C2, c.HW).permute(0, 2, 1, 3).contiguous()
    return skip, res


def join_values(c, planted=None):
    """v fp32 [rows][C2], the residual gathered by the kernel's own index arithmetic.  planted: layout_swapped (4-D strides on a 5-D
    residual and the reverse), bf_swapped (n % F as the clip, n / F as the frame)"""
    skip, res = join_problem(c.id)
    if res is None:
        return skip.clone()
    five = (c.res == "5d") != (planted == "layout_swapped")
    fb, ff, ch = c.F * c.C2 * c.HW, (c.HW if five else c.C2 * c.HW), (c.F * c.HW if five else c.HW)
    n = torch.arange(c.B * c.F)
    b_, f_ = (n % c.F, n // c.F) if planted == "bf_swapped" else (n // c.F, n % c.F)
    idx = (b_ * fb + f_ * ff)[:, None, None] + torch.arange(c.HW)[None, :, None] + (torch.arange(c.C2) * ch)[None, None, :]
    flat = res.reshape(-1).float()
    return skip + flat[idx % flat.numel()].reshape(-1, c.C2)


def join_mirror(c, v, planted=None):
    """the whole fp16 mirror [rows][ld_out | 2 ld_out], poison where nothing is written.  planted: lo_zero, lo_shifted (lo at lo_off - 8)"""
    rows = v.shape[0]
    split = c.mirror == "split"
    buf = torch.full((rows, (2 if split else 1) * c.ld_out), POISON[F16], dtype=F16)
    hi = v.half()
    buf[:, c.col:c.col + c.C2] = hi
    if split:
        lo = (v - hi.float()).half()
        off = c.lo_off - (8 if planted == "lo_shifted" else 0) + c.col
        buf[:, off:off + c.C2] = torch.zeros_like(lo) if planted == "lo_zero" else lo
    return buf


# ---------------------------------------------------------------------------------------------------------------------------
# vae_posterior
# ---------------------------------------------------------------------------------------------------------------------------
PO_SHAPES = ((1, 255), (1, 256), (1, 257), (3, 100))          # (N, hw)
PO_LATS = (1, 3, 4, 8)
PO_LV = (-45.0, -30.0, -0.5, 20.0, 31.0)          # the logvar before its clamp, planted
PO_SCALES = (1.0, 0.18215)
PO_WQ = ("both", "wq", "none")
POSTERIOR = []
for _lat in PO_LATS:
    for _i in range(18):
        _N, _hw = PO_SHAPES[_i % 4]
        POSTERIOR.append(Case(id="po-lat%d-N%dhw%d-%s-%s-%s-eps%s-out%s-s%g" % (
            _lat, _N, _hw, ("mode", "sample", "moments")[_i % 3], ("rows", "nchw")[(_i + _i // 4) % 2], PO_WQ[(_i + _i // 3) % 3],
            DT_NAME[DTYPES[(_i // 3 + _i // 9) % 3]], DT_NAME[DTYPES[(_i // 3) % 3]], PO_SCALES[(_i // 3 + _i // 6) % 2]),
            lat=_lat, N=_N, hw=_hw, kind=_i % 3, nchw=(_i + _i // 4) % 2, wq=PO_WQ[(_i + _i // 3) % 3], eps_dt=DTYPES[(_i // 3 + _i // 9) % 3],
            out_dt=DTYPES[(_i // 3) % 3], scale=PO_SCALES[(_i // 3 + _i // 6) % 2], ldx=2 * _lat + (3 if (_i + _i // 4) % 2 else 8)))
PO_BY_ID = {c.id: c for c in POSTERIOR}


@functools.lru_cache(maxsize=None)
def posterior_problem(case_id):
    """xbuf fp32 (rows: [N hw][ldx]; NCHW: [N][ldx][hw]; the surplus columns / channels NaN), wq [2 lat][2 lat] or None, bq or None, eps
    [N][lat][hw] in eps_dt.  x is solved so that q = bq + wq x meets drawn moments whose logvar holds PO_LV at the first and last pixels"""
    c = PO_BY_ID[case_id]
    g = _gen("po", case_id)
    n, C2 = c.N * c.hw, 2 * c.lat
    m = torch.cat([torch.randn(n, c.lat, generator=g, dtype=torch.float64) * 2.0, torch.randn(n, c.lat, generator=g, dtype=torch.float64) * 1.5], 1)
    for j in range(5 * c.lat):
        m[j, c.lat + j % c.lat] = PO_LV[j % 5]
        m[n - 1 - j, c.lat + (j + 1) % c.lat] = PO_LV[(j + 2) % 5]
    wq = bq = None
    if c.wq != "none":
        wq = torch.eye(C2) + 0.3 * torch.randn(C2, C2, generator=g) / math.sqrt(C2)
        bq = torch.randn(C2, generator=g) * 0.5 if c.wq == "both" else None
        m = torch.linalg.solve(wq.double(), (m - (bq.double() if bq is not None else 0.0)).t()).t()
    x = m.float()
    if c.nchw:
        xbuf = torch.full((c.N, c.ldx, c.hw), float("nan"))
        xbuf[:, :C2] = x.reshape(c.N, c.hw, C2).permute(0, 2, 1)
    else:
        xbuf = torch.full((n, c.ldx), float("nan"))
        xbuf[:, :C2] = x
    eps = torch.randn(c.N, c.lat, c.hw, generator=g).clamp(-2.0, 2.0).to(c.eps_dt)
    return xbuf, wq, bq, eps


def _po_x(c, xbuf, planted=None):
    """x [N hw][2 lat] as the kernel reads it; planted nchw_stride: the image stride 2 lat instead of ldx"""
    C2, n = 2 * c.lat, c.N * c.hw
    if not c.nchw:
        return xbuf[:, :C2]
    ld = C2 if planted == "nchw_stride" else c.ldx
    i = torch.arange(n)
    idx = ((i // c.hw) * ld)[:, None] * c.hw + torch.arange(C2)[None, :] * c.hw + (i % c.hw)[:, None]
    return xbuf.reshape(-1)[idx]


def _po_layout(c, planes):
    """planes: a list of [N hw][lat] tensors -> [N][len * lat][hw]"""
    return torch.cat([p.reshape(c.N, c.hw, c.lat).permute(0, 2, 1) for p in planes], 1).contiguous()


def posterior_moments64(c):
    """fp64 (mean, lv, std, var) and their bounds (d_mean, d_lv, d_std, d_var), each [N hw][lat]"""
    xbuf, wq, bq, _ = posterior_problem(c.id)
    x = _po_x(c, xbuf).double()
    if wq is None:
        q, dq = x, torch.zeros_like(x)
    else:
        b = bq.double() if bq is not None else torch.zeros(2 * c.lat, dtype=torch.float64)
        q = x @ wq.double().t() + b
        dq = (2 * c.lat + 2) * U * (x.abs() @ wq.double().abs().t() + b.abs())
    mean, lv = q[:, :c.lat], q[:, c.lat:].clamp(-30.0, 20.0)
    dmean, dlv = dq[:, :c.lat], dq[:, c.lat:]
    std, var = torch.exp(0.5 * lv), torch.exp(lv)
    dstd = std * (0.5 * dlv + PO_E * U * (1.0 + (0.5 * lv).abs()))
    dvar = var * (dlv + PO_E * U * (1.0 + lv.abs()))
    return (mean, lv, std, var), (dmean, dlv, dstd, dvar)


def posterior_prelogvar(c):
    """fp64: the logvar before its clamp, [N hw][lat]"""
    xbuf, wq, bq, _ = posterior_problem(c.id)
    x = _po_x(c, xbuf).double()
    if wq is not None:
        x = x @ wq.double().t() + (bq.double() if bq is not None else 0.0)
    return x[:, c.lat:]


def posterior_reference(c):
    """ref, bound fp64 in the output's layout: [N][lat][hw], MOMENTS [N][4 lat][hw]"""
    _, _, _, eps = posterior_problem(c.id)
    (mean, lv, std, var), (dmean, dlv, dstd, dvar) = posterior_moments64(c)
    s = float(_f32(c.scale))
    if c.kind == MOMENTS:
        ref, b = _po_layout(c, [mean, lv, std, var]), _po_layout(c, [dmean, dlv, dstd, dvar])
    elif c.kind == PSAMPLE:
        e = eps.double().permute(0, 2, 1).reshape(c.N * c.hw, c.lat)
        pre = std * e + mean
        ref = _po_layout(c, [pre * s])
        b = _po_layout(c, [(dstd * e.abs() + dmean + U * pre.abs()) * abs(s)]) + U * ref.abs()
    else:
        ref = _po_layout(c, [mean * s])
        b = _po_layout(c, [dmean * abs(s)]) + U * ref.abs()
    return ref, b + out_quantum(ref, c.out_dt) + TINY


def overflow_check(out, ref, bound, dt):
    """HF.check, but an fp16 result whose reference lies at or beyond 65520 must be that infinity"""
    o = out.double()
    if dt != F16:
        return check(out, ref, bound)
    ovf = ref.abs() >= FP16_OVF
    if not bool((o[ovf] == torch.sign(ref[ovf]) * float("inf")).all()) or not bool(torch.isfinite(o[~ovf]).all()):
        return float("inf")
    return float(((o[~ovf] - ref[~ovf]).abs() / bound[~ovf]).max())


def posterior_emulate(c, planted=None, kind=None, out_dt=None):
    """planted: clamp30 (the upper clamp at 30), std_explv (std = exp(lv)), no_bq, nchw_stride, noise_unscaled (the scale on the mean only)"""
    xbuf, wq, bq, eps = posterior_problem(c.id)
    kind = c.kind if kind is None else kind
    out_dt = c.out_dt if out_dt is None else out_dt
    v = _po_x(c, xbuf, planted)
    C2 = 2 * c.lat
    if wq is None:
        q = v
    else:
        q = (bq if (bq is not None and planted != "no_bq") else torch.zeros(C2))[None, :].expand(v.shape[0], C2)
        for ci in range(C2):
            q = _fma(wq[:, ci][None, :], v[:, ci, None], q)
    mean, lv = q[:, :c.lat], q[:, c.lat:].clamp(-30.0, 30.0 if planted == "clamp30" else 20.0)
    std = torch.exp(lv if planted == "std_explv" else _f32(0.5) * lv)
    s = _f32(c.scale)
    if kind == MOMENTS:
        return _po_layout(c, [mean, lv, std, torch.exp(lv)]).to(out_dt)
    if kind == PSAMPLE:
        e = eps.float().permute(0, 2, 1).reshape(c.N * c.hw, c.lat)
        r = _fma(std, e, mean * s) if planted == "noise_unscaled" else _fma(std, e, mean) * s
        return _po_layout(c, [r]).to(out_dt)
    return _po_layout(c, [mean * s]).to(out_dt)


# ---------------------------------------------------------------------------------------------------------------------------
# vae_dec_head
# ---------------------------------------------------------------------------------------------------------------------------
HD_MAPS, HD_COUTS, HD_LATS = ((1, 1), (1, 9), (9, 1), (5, 17), (13, 21)), (16, 48, 128), (1, 4, 8)
HEAD = []
for _i, ((_h, _w), _Co, _lat) in enumerate((m, o, l) for m in HD_MAPS for o in HD_COUTS for l in HD_LATS):
    _dt, _fr = DTYPES[(_i + _i // 3) % 3], (1, 3)[(_i // 2 + _i // 9) % 2]
    HEAD.append(Case(id="hd-%dx%d-Co%d-lat%d-%s-%s" % (_h, _w, _Co, _lat, DT_NAME[_dt], "dense" if _fr == 1 else "clip"), h=_h, w=_w, Cout=_Co,
                     lat=_lat, dt=_dt, frames=_fr, scale=(1.0 / 0.13025, 1.0 / 0.18215)[_i % 2]))
HD_BY_ID = {c.id: c for c in HEAD}


@functools.lru_cache(maxsize=None)
def head_problem(case_id):
    """clip [lat][frames][h][w] of c.dt (the latents are frame frames // 2, the other frames NaN), wpq [lat][lat], bpq [lat] (about 1: far
    from 0), w fp32 [Cout][lat][3][3], b [Cout], ref, bound fp64 [h w][Cout]"""
    c = HD_BY_ID[case_id]
    g = _gen("hd", case_id)
    z = torch.randn(c.lat, c.h, c.w, generator=g).to(c.dt)
    clip = torch.full((c.lat, c.frames, c.h, c.w), float("nan"), dtype=c.dt)
    clip[:, c.frames // 2] = z
    wpq = torch.randn(c.lat, c.lat, generator=g) * 0.5
    bpq = 1.0 + 0.3 * torch.randn(c.lat, generator=g)
    w = torch.randn(c.Cout, c.lat, 3, 3, generator=g) / math.sqrt(9.0 * c.lat)
    b = torch.randn(c.Cout, generator=g) * 0.1
    s = float(_f32(c.scale))
    two = lambda zz, a, ab, ww, bb: Fn.conv2d(Fn.conv2d(zz[None], a[:, :, None, None], ab), ww, bb, padding=1)[0]
    ref = two(z.double() * s, wpq.double(), bpq.double(), w.double(), b.double())
    mag = two(z.double().abs() * abs(s), wpq.double().abs(), bpq.double().abs(), w.double().abs(), b.double().abs())
    f = lambda t: t.permute(1, 2, 0).reshape(c.h * c.w, c.Cout)
    return clip, wpq, bpq, w, b, f(ref), f((9 * c.lat + c.lat + 4) * U * mag)


def head_emulate(case_id, planted=None):
    """q = bpq, lat fmas over ci, per tapped pixel; acc = b, fmas in (tap, o) order over the taps inside the map.
    planted: bpq_outside (z padded instead of q: q = bpq outside the map), scale_after (the scale on q instead of z), clip_stride (the
    channel stride h w for a frame of a clip)"""
    c = HD_BY_ID[case_id]
    clip, wpq, bpq, w, b, _, _ = head_problem(case_id)
    hw = c.h * c.w
    cs = hw if planted == "clip_stride" else c.frames * hw
    idx = (c.frames // 2) * hw + torch.arange(c.lat)[:, None] * cs + torch.arange(hw)[None, :]
    z = clip.reshape(-1)[idx].float().reshape(c.lat, c.h, c.w)
    s = _f32(c.scale)
    v = z if planted == "scale_after" else z * s
    q = []
    for o in range(c.lat):
        a = bpq[o].expand(c.h, c.w)
        for ci in range(c.lat):
            a = _fma(wpq[o, ci], v[ci], a)
        q.append(a * s if planted == "scale_after" else a)
    q = torch.stack(q)
    qp = Fn.pad(q, (1, 1, 1, 1))
    if planted == "bpq_outside":
        qp = bpq[:, None, None].expand(c.lat, c.h + 2, c.w + 2).clone()
        qp[:, 1:-1, 1:-1] = q
    acc = b[None, None, :].expand(c.h, c.w, c.Cout)
    for t in range(9):
        for o in range(c.lat):
            acc = _fma(w[:, o, t // 3, t % 3][None, None, :], qp[o, t // 3:t // 3 + c.h, t % 3:t % 3 + c.w, None], acc)
    return acc.reshape(hw, c.Cout)


# ---------------------------------------------------------------------------------------------------------------------------
# vae_dec_tail
# ---------------------------------------------------------------------------------------------------------------------------
TL_WS, TL_HS, TL_CS, TL_COUTS = (1, 31, 32, 33, 65), (1, 7, 8, 9, 17), (32, 64, 96, 160), (1, 2, 3, 4)
TL_EPS = 1e-6
TL_FLAT_VALUE = 5.3          # the constant of the `flat` case's channel group (see tail_problem)
TAIL = []
for _i, (_H, _W) in enumerate([(9, w) for w in TL_WS] + [(h, 33) for h in TL_HS if h != 9]):
    TAIL.append(Case(id="tl-%dx%d-C%d-Co%d" % (_H, _W, TL_CS[_i % 4], TL_COUTS[(_i + _i // 4) % 4]), H=_H, W=_W, C=TL_CS[_i % 4],
                     Cout=TL_COUTS[(_i + _i // 4) % 4], flat=None, tie=None))
for _Co in TL_COUTS:          # every template at C = 96 (cg = 3, three chunks), on a map of two tiles each way
    TAIL.append(Case(id="tl-9x33-C96-Co%d-all" % _Co, H=9, W=33, C=96, Cout=_Co, flat=None, tie=None))
TAIL.append(Case(id="tl-9x33-C96-Co3-flat", H=9, W=33, C=96, Cout=3, flat=5, tie=None))          # group 5 constant over the whole map
TAIL.append(Case(id="tl-7x33-C32-Co2-tie", H=7, W=33, C=32, Cout=2, flat=None, tie=126))            # output channel 0: zero weights, u * 255 = 126.5
TL_BY_ID = {c.id: c for c in TAIL}


def tie_bias(k):
    """v with fp32(fp32(v / 2 + 0.5) * 255) == k + 0.5 exactly (k >= 64: u = v / 2 + 0.5 >= 0.25 and v are then both exact in fp32)"""
    u = _f32((k + 0.5) / 255.0)
    for step in range(-8, 9):
        uu = (u.view(torch.int32) + step).view(F32)
        if float(uu * _f32(255.0)) == k + 0.5:
            v = uu * 2.0 - 1.0
            assert float(v * _f32(0.5) + _f32(0.5)) == float(uu)
            return float(v)
    raise AssertionError("no fp32 u with u * 255 == %g" % (k + 0.5))


@functools.lru_cache(maxsize=None)
def tail_problem(case_id):
    """x fp32 [H][W][C], stats fp32 [64] (sum, sum of squares per group: the fp32 roundings of the fp64 sums), gamma, beta (chosen so that beta - mean sc is about 1:
    the activated value of a zero-padded x, silu of that, is far from 0), w fp32 [Cout][C][3][3], b [Cout].
    flat: one group holds TL_FLAT_VALUE everywhere; its two sums are exact in fp32, the fp32 variance ss / n - mean^2 is not 0."""
    c = TL_BY_ID[case_id]
    g = _gen("tl", case_id)
    x = torch.randn(c.H, c.W, c.C, generator=g) * 1.5 + 0.3 + 0.5 * torch.randn(c.C, generator=g)[None, None, :]
    cg = c.C // 32
    if c.flat is not None:
        x[:, :, c.flat * cg:(c.flat + 1) * cg] = TL_FLAT_VALUE
    s, ss = NF.gn_sums(x.double().reshape(1, c.H * c.W, c.C), 32)
    stats = torch.stack([s[0], ss[0]], 1).reshape(-1).float()
    gamma = 1.0 + 0.1 * torch.randn(c.C, generator=g)
    n = c.H * c.W * cg
    mean = s[0] / n
    rstd = 1.0 / torch.sqrt((ss[0] / n - mean * mean).clamp_min(0.0) + TL_EPS)
    beta = (1.0 + 0.1 * torch.randn(c.C, generator=g) + ((mean * rstd).repeat_interleave(cg) * gamma.double())).float()          # beta - mean sc about 1
    w = torch.randn(c.Cout, c.C, 3, 3, generator=g) * (3.0 / math.sqrt(9.0 * c.C))
    b = torch.randn(c.Cout, generator=g) * 0.1
    if c.tie is not None:
        w[0] = 0.0
        b[0] = tie_bias(c.tie)
    return x, stats, gamma, beta, w, b


@functools.lru_cache(maxsize=None)
def tail_reference(case_id):
    """ref, bound fp64 [1][Cout][H][W] of the fp32 SAMPLE"""
    c = TL_BY_ID[case_id]
    x, stats, gamma, beta, w, b = tail_problem(case_id)
    st = stats.double().reshape(32, 2)
    n = c.H * c.W * (c.C // 32)
    pre, bpre = NF.gn_out(x.double().reshape(1, c.H * c.W, c.C), st[None, :, 0], st[None, :, 1], n, gamma, beta, 32, False, eps=TL_EPS)
    dpre = bpre - NF.ulp16(pre)
    act = NF.silu64(pre)
    dact = 1.1 * dpre + HF._equick(pre.abs() + dpre, pre)
    img = lambda t: t.reshape(1, c.H, c.W, c.C).permute(0, 3, 1, 2)
    ref = Fn.conv2d(img(act), w.double(), b.double(), padding=1)
    mag = Fn.conv2d(img(act.abs()), w.double().abs(), b.double().abs(), padding=1)
    bound = Fn.conv2d(img(dact), w.double().abs(), padding=1) + (9 * c.C + 2) * U * mag
    return ref, bound


def tail_scales(c, stats, gamma, beta, planted=None):
    """(sc, sf, var before the clamp) fp32 [C], the arithmetic of the kernel's first 32 lanes; planted: group_c32 (group c / 32), unclamped"""
    cg = c.C // 32
    inv_cnt = _f32(1.0) / (_f32(float(c.H)) * _f32(float(c.W)) * _f32(float(cg)))
    ch = torch.arange(c.C)
    gidx = ch // 32 if planted == "group_c32" else ch // cg
    st = stats.reshape(32, 2)
    s, ss = st[gidx, 0], st[gidx, 1]
    mean = s * inv_cnt
    var0 = ss * inv_cnt - mean * mean
    var = var0 if planted == "unclamped" else var0.clamp_min(0.0)
    sc = torch.rsqrt(var + _f32(TL_EPS)) * gamma
    return sc, beta - mean * sc, var0


def tail_emulate(case_id, planted=None):
    """the fp32 SAMPLE [1][Cout][H][W]: acc = 0, then chunk by chunk, tap by tap, channel by channel one fma; + b at the end.
    planted: pad_before_act (x padded, then normalised and activated), first_chunk_scales (chunk 0's sc / sf for every chunk), group_c32,
    no_halo_x32 (the patch column of x = 32 empty for the tile that ends at x = 31), unclamped"""
    c = TL_BY_ID[case_id]
    x, stats, gamma, beta, w, b = tail_problem(case_id)
    sc, sf, _ = tail_scales(c, stats, gamma, beta, planted)
    if planted == "first_chunk_scales":
        sc, sf = sc[:TAIL_CK].repeat(c.C // TAIL_CK), sf[:TAIL_CK].repeat(c.C // TAIL_CK)
    silu = lambda f: f * (1.0 / (1.0 + torch.exp(-f)))
    if planted == "pad_before_act":
        act = silu(_fma(Fn.pad(x, (0, 0, 1, 1, 1, 1)), sc, sf))
    else:
        act = Fn.pad(silu(_fma(x, sc, sf)), (0, 0, 1, 1, 1, 1))          # [H + 2][W + 2][C]
    acc = torch.zeros(c.H, c.W, c.Cout)
    for c0 in range(0, c.C, TAIL_CK):
        for t in range(9):
            a = act[t // 3:t // 3 + c.H, t % 3:t % 3 + c.W]
            if planted == "no_halo_x32" and t % 3 == 2 and c.W > TAIL_W:
                a = a.clone()
                a[:, TAIL_W - 1] = 0.0          # the pixel at x = 31 reads its right neighbour, x = 32
            for ch in range(c0, c0 + TAIL_CK):
                acc = _fma(w[:, ch, t // 3, t % 3][None, None, :], a[:, :, ch, None], acc)
    return (acc + b).permute(2, 0, 1)[None].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# vae_time_conv
# ---------------------------------------------------------------------------------------------------------------------------
TC_OCS, TC_FS = (1, 2, 3, 4), (1, 3, 4, 5, 8, 9)
TC_HW_VEC, TC_HW_SCALAR = (4, 1020, 1024, 1028), (1, 255, 257, 1026)
TIME_CONV = [Case(id="tc-OC%d-F%d-HW%d" % (oc, f, hw), OC=oc, F=f, HW=hw, vec=hw % TC_PV == 0)
             for oc in TC_OCS for f in TC_FS for hw in TC_HW_VEC + TC_HW_SCALAR]
TC_BY_ID = {c.id: c for c in TIME_CONV}
TC_KINDS = [(k, d) for k in (SAMPLE, UNIT, BYTES) for d in DTYPES]
TC_KIND_CASES = ("tc-OC3-F5-HW1028", "tc-OC3-F5-HW1026")
# what sends vector-shaped data down the scalar kernel: (name, byte offset of x, kind, dtype, byte offset of out)
TC_MISALIGN = (("x + 4", 4, SAMPLE, F32, 0), ("f32 out + 4", 0, SAMPLE, F32, 4), ("unit out + 4", 0, UNIT, F16, 4), ("f16 out + 4", 0, SAMPLE, F16, 4),
               ("bf16 out + 4", 0, SAMPLE, BF16, 4), ("u8 out + 1", 0, BYTES, F32, 1), ("u8 out + 2", 0, BYTES, F32, 2))
TC_MISALIGN_CASES = ("tc-OC3-F5-HW1028", "tc-OC4-F9-HW1024", "tc-OC1-F4-HW4", "tc-OC2-F8-HW1020")


@functools.lru_cache(maxsize=None)
def time_conv_problem(case_id):
    """x fp32 [F][OC][HW], w [OC][OC][3] (o, c, t), b [OC], ref, bound fp64 [F][OC][HW]"""
    c = TC_BY_ID[case_id]
    g = _gen("tc", case_id)
    x = torch.randn(c.F, c.OC, c.HW, generator=g) * 1.5
    w = torch.randn(c.OC, c.OC, 3, generator=g) * 0.5
    b = torch.randn(c.OC, generator=g) * 0.1
    one = lambda xx, ww, bb: Fn.conv1d(xx.permute(2, 1, 0), ww, bb, padding=1).permute(2, 1, 0)          # [HW][OC][F] over the frames
    ref = one(x.double(), w.double(), b.double())
    mag = one(x.double().abs(), w.double().abs(), b.double().abs())
    return x, w, b, ref, (3 * c.OC + 2) * U * mag


def time_conv_emulate(case_id, planted=None):
    """acc = b, then fmas in (c, t) order; planted: seam_zero (the frames outside a group of kTcFrames read as zero), taps_reversed,
    w_transposed ((c, o) for (o, c))"""
    c = TC_BY_ID[case_id]
    x, w, b, _, _ = time_conv_problem(case_id)
    if planted == "w_transposed":
        w = w.transpose(0, 1)
    if planted == "taps_reversed":
        w = w.flip(2)
    xp = Fn.pad(x, (0, 0, 0, 0, 1, 1))          # frames -1 .. F
    f = torch.arange(c.F)
    acc = b[None, :, None].expand(c.F, c.OC, c.HW)
    for ci in range(c.OC):
        for t in range(3):
            src = xp[f + t, ci]
            if planted == "seam_zero":
                src = src * ((f + t - 1) // TC_FRAMES == f // TC_FRAMES).float()[:, None]
            acc = _fma(w[:, ci, t][None, :, None], src[:, None, :], acc)
    return acc


# ---------------------------------------------------------------------------------------------------------------------------
# i2v_latent_encoder
# ---------------------------------------------------------------------------------------------------------------------------
ENC_FS = (1, 2, 3, 5, 7, 16, 31, 32)
ENC_KINDS = ("plain", "saturated", "equal")
ENC_ALL_DT = (3, 32)
ENC_SAT = 16.0         # the saturated kind's to_q and to_k are this much larger
ENC_OFF = {"g": 0, "b": 4, "q": 8, "k": 40, "v": 72, "o": 104, "bo": 136, "w1": 140, "b1": 204, "w2": 220, "b2": 284}
ENCODER = []
for _F in ENC_FS:
    _P = enc_P(_F)
    for _j, _np in enumerate((_P - 1, _P, _P + 1, 2 * _P + 1)):
        if _np < 1:
            continue
        _B = 2 if _np % 2 == 0 else 1
        for _k, _dt in enumerate(DTYPES if _F in ENC_ALL_DT else (F32,)):
            ENCODER.append(Case(id="enc-F%d-npix%d-B%d-%s-%s" % (_F, _np, _B, DT_NAME[_dt], ENC_KINDS[(_j + _k) % 3]), F=_F, P=_P, npix=_np, B=_B,
                                HW=_np // _B, dt=_dt, kind=ENC_KINDS[(_j + _k) % 3]))
ENC_BY_ID = {c.id: c for c in ENCODER}


@functools.lru_cache(maxsize=None)
def enc_weights(saturated):
    """the 288 floats in ctrl_op_i2v_latent_encoder's order"""
    g = _gen("enc-w")
    w = torch.zeros(ENC_WTS)
    w[0:4] = 1.0 + 0.1 * torch.randn(4, generator=g)
    w[4:8] = 0.1 * torch.randn(4, generator=g)
    w[8:104] = torch.randn(96, generator=g) * 0.5
    w[104:136] = torch.randn(32, generator=g) / math.sqrt(8.0)
    w[136:140] = 0.1 * torch.randn(4, generator=g)
    w[140:204] = torch.randn(64, generator=g) * 0.5
    w[204:220] = 0.1 * torch.randn(16, generator=g)
    w[220:284] = torch.randn(64, generator=g) * 0.25
    w[284:288] = 0.1 * torch.randn(4, generator=g)
    if saturated:
        w[8:72] *= ENC_SAT
    return w


def enc_state_dict(w):
    """the 288 floats as the state dict of unet_i2vgen_ref.LatentTemporalEncoderRef(4, 2, 4, 16)"""
    return {"norm1.weight": w[0:4], "norm1.bias": w[4:8], "attn1.to_q.weight": w[8:40].reshape(8, 4), "attn1.to_k.weight": w[40:72].reshape(8, 4),
            "attn1.to_v.weight": w[72:104].reshape(8, 4), "attn1.to_out.0.weight": w[104:136].reshape(4, 8), "attn1.to_out.0.bias": w[136:140],
            "ff.net.0.proj.weight": w[140:204].reshape(16, 4), "ff.net.0.proj.bias": w[204:220], "ff.net.2.weight": w[220:284].reshape(4, 16),
            "ff.net.2.bias": w[284:288]}


@functools.lru_cache(maxsize=None)
def enc_problem(case_id):
    """x fp32 rows [(b f) p][4], wts [288], sample [B][4][F][HW] in c.dt"""
    c = ENC_BY_ID[case_id]
    g = _gen("enc", case_id)
    x = torch.randn(c.B, c.F, c.HW, 4, generator=g)
    if c.kind == "equal":
        x = x[:, :1].expand(c.B, c.F, c.HW, 4)
    x = x.reshape(c.B * c.F * c.HW, 4).contiguous()
    sample = HF.odd_values((c.B, 4, c.F, c.HW), c.dt, g)
    return x, enc_weights(c.kind == "saturated"), sample


def enc_tokens(c, rows):
    """rows [(b f) p][n] -> tokens [(b p)][f][n], and back"""
    return rows.reshape(c.B, c.F, c.HW, -1).permute(0, 2, 1, 3).reshape(c.npix, c.F, -1)


def enc_rows(c, tok):
    return tok.reshape(c.B, c.HW, c.F, -1).permute(0, 2, 1, 3).reshape(c.B * c.F * c.HW, -1)


def enc_sample_rows(c, sample):
    """columns 0..3: the sample converted once, row (b f) p <- sample[b, c, f, p]"""
    return sample.float().permute(0, 2, 3, 1).reshape(c.B * c.F * c.HW, 4).contiguous()


@functools.lru_cache(maxsize=None)
def enc_reference(case_id):
    """ref, bound fp64 rows [(b f) p][4] (the derivation is in the header), the score spread and the largest weight per (token, head,
    query), the scores [n][2][F][F] and the feed-forward's pre-activations [n][F][16]"""
    c = ENC_BY_ID[case_id]
    x, wts, _ = enc_problem(case_id)
    w = wts.double()
    K, Fr = EN_K, c.F
    xt = enc_tokens(c, x.double())                                    # [n][F][4]
    g, b = w[0:4], w[4:8]
    Wq, Wk, Wv, Wo, bo = w[8:40].reshape(8, 4), w[40:72].reshape(8, 4), w[72:104].reshape(8, 4), w[104:136].reshape(4, 8), w[136:140]
    W1, b1, W2, b2 = w[140:204].reshape(16, 4), w[204:220], w[220:284].reshape(4, 16), w[284:288]
    mean = xt.mean(-1, keepdim=True)
    mabs = xt.abs().mean(-1, keepdim=True)
    d = xt - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xn = d * rstd * g + b
    dd = K * U * (mabs + xt.abs())
    rho = (d.abs() * dd).sum(-1, keepdim=True) / (4.0 * (var + 1e-5)) + K * U
    dxn = (dd * rstd + d.abs() * rstd * rho) * g.abs() + K * U * xn.abs()
    lin = lambda W, v, dv, k: (v @ W.t(), dv @ W.abs().t() + k * U * (v.abs() @ W.abs().t()))
    q, dq = lin(Wq, xn, dxn, 5)
    k, dk = lin(Wk, xn, dxn, 5)
    v, dv = lin(Wv, xn, dxn, 5)
    heads = lambda t: t.reshape(c.npix, Fr, 2, 4).permute(0, 2, 1, 3)          # [n][2][F][4]
    qh, kh, vh, dqh, dkh, dvh = (heads(t) for t in (q, k, v, dq, dk, dv))
    s = 0.5 * qh @ kh.transpose(-1, -2)                                        # [n][2][Fq][Fk]
    ds = 0.5 * (qh.abs() @ dkh.transpose(-1, -2) + dqh @ kh.abs().transpose(-1, -2)) + 5 * U * 0.5 * (qh.abs() @ kh.abs().transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    wt = torch.softmax(s, -1)
    dw = wt * (ds + (wt * ds).sum(-1, keepdim=True) + K * U * (1.0 + (s - m).abs()) + (Fr + 2) * U)
    o = wt @ vh
    do = dw @ vh.abs() + wt @ dvh + (Fr + 2) * U * (wt @ vh.abs())
    unheads = lambda t: t.permute(0, 2, 1, 3).reshape(c.npix, Fr, 8)
    o, do = unheads(o), unheads(do)
    x1 = o @ Wo.t() + bo + xt
    dx1 = do @ Wo.abs().t() + 11 * U * (o.abs() @ Wo.abs().t() + bo.abs() + xt.abs())
    a = x1 @ W1.t() + b1
    da = dx1 @ W1.abs().t() + 6 * U * (x1.abs() @ W1.abs().t() + b1.abs())
    h = 0.5 * a * (1.0 + torch.special.erf(a / math.sqrt(2.0)))
    dh = 1.13 * da + K * U * (a.abs() + da)
    out = h @ W2.t() + b2 + x1
    dout = dh @ W2.abs().t() + 19 * U * (h.abs() @ W2.abs().t() + b2.abs() + x1.abs()) + dx1
    return enc_rows(c, out), enc_rows(c, dout), (s.max(-1).values - s.min(-1).values), wt.max(-1).values, s, a


def enc_stage_shares(case_id):
    """What EN_K is calibrated on: each non-linear stage alone, its fp32 emulation on fp32 inputs against the fp64 value of the same
    inputs and the stage's own term of the bound -> (LayerNorm, softmax weights, erf GELU).  (On the whole chain the derived fma-chain
    terms, which take every product at its absolute value through five layers, hold most of the bound: it cannot tell EN_K.)"""
    c = ENC_BY_ID[case_id]
    x, wts, _ = enc_problem(case_id)
    w, K, Fr = wts.double(), EN_K, c.F
    xt32 = enc_tokens(c, x)
    xt = xt32.double()
    g, b = w[0:4], w[4:8]
    mean, mabs = xt.mean(-1, keepdim=True), xt.abs().mean(-1, keepdim=True)
    d = xt - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xn = d * rstd * g + b
    dd = K * U * (mabs + xt.abs())
    rho = (d.abs() * dd).sum(-1, keepdim=True) / (4.0 * (var + 1e-5)) + K * U
    dxn = (dd * rstd + d.abs() * rstd * rho) * g.abs() + K * U * xn.abs()
    m32 = ((xt32[..., 0] + xt32[..., 1]) + (xt32[..., 2] + xt32[..., 3])) * _f32(0.25)
    d32 = xt32 - m32[..., None]
    v32 = ((d32[..., 0] * d32[..., 0] + d32[..., 1] * d32[..., 1]) + (d32[..., 2] * d32[..., 2] + d32[..., 3] * d32[..., 3])) * _f32(0.25)
    xn32 = d32 * (_f32(1.0) / torch.sqrt(v32 + _f32(1e-5)))[..., None] * wts[0:4] + wts[4:8]
    ln = float(((xn32.double() - xn).abs() / dxn).max())
    # the weights of the fp32-rounded scores of the reference
    s32 = enc_reference(case_id)[4].float()
    s = s32.double()
    mx = s.max(-1, keepdim=True).values
    wt = torch.softmax(s, -1)
    e32 = torch.exp(s32 - s32.max(-1, keepdim=True).values)
    w32 = e32 / NF._seq_sum(e32, 3)[..., None]
    sm = float(((w32.double() - wt).abs() / (wt * (K * U * (1.0 + (s - mx).abs()) + (Fr + 2) * U) + 2.0 ** -126)).max())
    a32 = enc_reference(case_id)[5].float()
    a = a32.double()
    h = 0.5 * a * (1.0 + torch.special.erf(a / math.sqrt(2.0)))
    h32 = _f32(0.5) * a32 * (1.0 + torch.erf(a32 * _f32(0.70710678118654752)))
    ge = float(((h32.double() - h).abs() / (K * U * a.abs() + 2.0 ** -126)).max())
    return ln, sm, ge


def enc_emulate(case_id, planted=None):
    """fp32 rows [(b f) p][4] in the kernel's association, the keys and values met through the workgroup's slots f * P + pl.
    planted: scale_one (softmax scale 1), extra_key (F + 1 keys: the slot behind the last frame's, an idle lane's: zeros here),
    stride_up (the reader's slot stride 256 / F rounded up), tanh_gelu, heads_swapped (the two heads' results exchanged before to_out)"""
    c = ENC_BY_ID[case_id]
    x, w, _ = enc_problem(case_id)
    Fr, P = c.F, c.P
    nwg = -(-c.npix // P)
    npad = nwg * P
    xt = NF._pad(enc_tokens(c, x), 0, npad)                          # the lanes of pixels beyond the batch hold zeros
    mean = ((xt[..., 0] + xt[..., 1]) + (xt[..., 2] + xt[..., 3])) * _f32(0.25)
    d = xt - mean[..., None]
    var = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3])) * _f32(0.25)
    rstd = _f32(1.0) / torch.sqrt(var + _f32(1e-5))
    xn = d * rstd[..., None] * w[0:4] + w[4:8]

    def chain(v, W, n):
        a = torch.zeros(v.shape[:-1] + (W.shape[0],))
        for i in range(n):
            a = _fma(v[..., i, None], W[:, i], a)
        return a

    q, k, v = chain(xn, w[8:40].reshape(8, 4), 4), chain(xn, w[40:72].reshape(8, 4), 4), chain(xn, w[72:104].reshape(8, 4), 4)
    # the key read as frame j of pixel n: slot j * stride + pl of the workgroup -> (pixel, frame) that wrote it, or nothing
    J = Fr + 1 if planted == "extra_key" else Fr
    stride = -(-THREADS // Fr) if planted == "stride_up" else P
    pix = torch.arange(npad)
    slot = torch.arange(J)[None, :] * stride + (pix % P)[:, None]                       # [npad][J]
    src_f, src_pl = slot // P, slot % P
    ok = (slot < THREADS) & (src_f < Fr)
    src_pix = (pix // P)[:, None] * P + src_pl
    kk = torch.where(ok[..., None], k[src_pix.clamp_max(npad - 1), src_f.clamp_max(Fr - 1)], torch.zeros(()))          # [npad][J][8]
    vv = torch.where(ok[..., None], v[src_pix.clamp_max(npad - 1), src_f.clamp_max(Fr - 1)], torch.zeros(()))
    sm = _f32(1.0 if planted == "scale_one" else 0.5)
    o8 = []
    for h in range(2):
        qh = q[:, :, None, h * 4:h * 4 + 4]                                               # [npad][F][1][4]
        kh = kk[:, None, :, h * 4:h * 4 + 4]                                              # [npad][1][J][4]
        sc = sm * (((qh[..., 0] * kh[..., 0] + qh[..., 1] * kh[..., 1]) + qh[..., 2] * kh[..., 2]) + qh[..., 3] * kh[..., 3])
        m = sc.max(-1, keepdim=True).values
        e = torch.exp(sc - m)
        den = NF._seq_sum(e, 2)
        a = torch.zeros(npad, Fr, 4)
        for j in range(J):
            a = _fma(e[:, :, j, None], vv[:, None, j, h * 4:h * 4 + 4], a)
        o8.append(a / den[..., None])
    o8 = torch.cat(o8[::-1] if planted == "heads_swapped" else o8, -1)
    x1 = (chain(o8, w[104:136].reshape(4, 8), 8) + w[136:140]) + xt
    a = chain(x1, w[140:204].reshape(16, 4), 4) + w[204:220]
    if planted == "tanh_gelu":
        hid = _f32(0.5) * a * (1.0 + torch.tanh(_f32(0.7978845608028654) * (a + _f32(0.044715) * a * a * a)))
    else:
        hid = _f32(0.5) * a * (1.0 + torch.erf(a * _f32(0.70710678118654752)))
    res = (chain(hid, w[220:284].reshape(4, 16), 16) + w[284:288]) + x1
    return enc_rows(c, res[:c.npix])


# ---------------------------------------------------------------------------------------------------------------------------
# adaptive_avgpool_nhwc
# ---------------------------------------------------------------------------------------------------------------------------
AAP_SHAPES = ((5, 7, 32, 32), (33, 47, 8, 16), (32, 32, 32, 32))          # (H, W, OH, OW)
AAP_ODD = ((9, 11, 3, 5, 7), (9, 11, 5, 7, 9))                           # + C: 2 * 15 * 7 = 210 and 2 * 35 * 9 = 630 outputs
AAPOOL = [Case(id="aap-%dx%d-%dx%d-C%d-N%d-%s-%s" % (s + (C, N, DT_NAME[xd], DT_NAME[yd])), H=s[0], W=s[1], OH=s[2], OW=s[3], C=C, N=N, x_dt=xd, y_dt=yd)
          for s in AAP_SHAPES for (C, N) in ((5, 1),) for xd in (F32, F16) for yd in (F32, F16)]
AAPOOL += [Case(id="aap-%dx%d-%dx%d-C%d-N2-%s-%s" % (s[:4] + (s[4], DT_NAME[xd], DT_NAME[yd])), H=s[0], W=s[1], OH=s[2], OW=s[3], C=s[4], N=2, x_dt=xd, y_dt=yd)
           for s in AAP_ODD for (xd, yd) in ((F32, F32), (F16, F16), (F16, F32))]


def aap_windows(n_in, n_out):
    return [((i * n_in) // n_out, -(-(i + 1) * n_in // n_out)) for i in range(n_out)]


def aap_problem(c):
    """x [N][H][W][C] of x_dt, ref, bound fp64 [N][OH][OW][C], one (True where the window holds one element: exact)"""
    x = HF.odd_values((c.N, c.H, c.W, c.C), c.x_dt, _gen("aap", c.id), 1.0)
    ref = Fn.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), (c.OH, c.OW)).permute(0, 2, 3, 1).contiguous()
    ky = torch.tensor([b - a for a, b in aap_windows(c.H, c.OH)])
    kx = torch.tensor([b - a for a, b in aap_windows(c.W, c.OW)])
    k = (ky[:, None] * kx[None, :]).double()[None, :, :, None].expand_as(ref)
    bound = (k + 1.0) * U * float(x.double().abs().max()) + out_quantum(ref, c.y_dt)
    return x, ref, bound, k == 1


def aap_emulate(c, planted=None):
    """planted: floor_end (the window's end floored instead of ceiled)"""
    x, _, _, _ = aap_problem(c)
    xf = x.float()
    out = torch.zeros(c.N, c.OH, c.OW, c.C)
    for oy, (y0, y1) in enumerate(aap_windows(c.H, c.OH)):
        for ox, (x0, x1) in enumerate(aap_windows(c.W, c.OW)):
            if planted == "floor_end":
                y1, x1 = max(y0 + 1, ((oy + 1) * c.H) // c.OH), max(x0 + 1, ((ox + 1) * c.W) // c.OW)
            acc = torch.zeros(c.N, c.C)
            for iy in range(y0, y1):
                for ix in range(x0, x1):
                    acc = acc + xf[:, iy, ix]
            out[:, oy, ox] = acc / _f32(float((y1 - y0) * (x1 - x0)))
    return out.to(c.y_dt)


# ---------------------------------------------------------------------------------------------------------------------------
# unet_text_time
# ---------------------------------------------------------------------------------------------------------------------------
TT_TEXT, TT_DIMS, TT_IDS, TT_BS = (1, 255, 256, 257, 1280), (2, 6, 256), (1, 6), (1, 3)
TT_PAD = 8          # poison columns between the rows
TEXT_TIME = []
for _i, (_td, _dim, _ni, _B) in enumerate((t, d, n, b) for t in TT_TEXT for d in TT_DIMS for n in TT_IDS for b in TT_BS):
    TEXT_TIME.append(Case(id="tt-text%d-dim%d-ids%d-B%d-%s" % (_td, _dim, _ni, _B, DT_NAME[DTYPES[(_i + _i // 4) % 3]]), text_dim=_td, dim=_dim, n_ids=_ni,
                          B=_B, dt=DTYPES[(_i + _i // 4) % 3]))


def tt_problem(c):
    """text [B][text_dim] of c.dt, ids fp32 [B][n_ids] (helper_forms.SC_TS, every row starting elsewhere), ref, bound fp64 [B][n_ids dim]"""
    text = HF.odd_values((c.B, c.text_dim), c.dt, _gen("tt", c.id))
    ids = torch.tensor([[HF.SC_TS[(b + i + c.text_dim) % 4] for i in range(c.n_ids)] for b in range(c.B)], dtype=F32)
    half = c.dim // 2
    k = torch.arange(half, dtype=torch.float64)
    xx = HF.LN1E4 * k / half
    arg = ids.double().reshape(-1)[:, None] * torch.exp(-xx)[None, :]
    darg = arg.abs() * (HF.SC_K * xx[None, :] + HF.SC_K) * U
    darg = torch.where((k == 0)[None, :], torch.zeros_like(darg), darg)
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1).reshape(c.B, c.n_ids * c.dim)
    bound = (torch.cat([darg, darg], 1) + HF.SC_C * U).reshape(c.B, c.n_ids * c.dim)
    return text, ids, ref, bound


def tt_emulate(c, planted=None):
    """planted: sin_cos (sin | cos), full_dim (dim instead of dim / 2 under the frequency's exponent)"""
    _, ids, _, _ = tt_problem(c)
    half = c.dim // 2
    k = torch.arange(half, dtype=F32)
    freq = torch.exp(_f32(-HF.LN1E4) * k / _f32(float(c.dim if planted == "full_dim" else half)))
    arg = ids.reshape(-1)[:, None] * freq[None, :]
    parts = [torch.sin(arg), torch.cos(arg)] if planted == "sin_cos" else [torch.cos(arg), torch.sin(arg)]
    return torch.cat(parts, 1).reshape(c.B, c.n_ids * c.dim)


# ---------------------------------------------------------------------------------------------------------------------------
# what the entry points refuse before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(ptr, odd_ptr):
    """[(name, symbol, ctypes argument list without the stream, part of the message)]: `ptr` any 16-byte aligned address the call may
    name (a refused call dereferences nothing), `odd_ptr` one that is 4 mod 16.  The stream goes last on every entry point."""
    import ctypes as C
    P, I, Q, F = (lambda: C.c_void_p(ptr)), C.c_int, C.c_int64, C.c_float
    null, odd = C.c_void_p(0), C.c_void_p(odd_ptr)

    def join(skip=None, out16=True, C2=32, ld_out=64, col=0, lo_off=32):
        return [skip or P(), Q(C2), null, I(0), I(0), I(1), I(1), I(4), I(C2), P(), P() if out16 else null, Q(ld_out), I(col), I(lo_off)]

    split_msg = "unet_skip_join: a split mirror's lo half"
    rows = [
        ("join lo_off % 8", "ctrl_op_unet_skip_join_split", join(lo_off=36), split_msg),
        ("join lo_off < col + C2", "ctrl_op_unet_skip_join_split", join(col=8, lo_off=32), split_msg),
        ("join lo beyond the row", "ctrl_op_unet_skip_join_split", join(ld_out=32, lo_off=40), split_msg),
        ("join lo_off without a mirror", "ctrl_op_unet_skip_join_split", join(out16=False), split_msg),
        ("join misaligned skip", "ctrl_op_unet_skip_join_split", join(skip=odd), "unet_skip_join: pointers must be 16-byte aligned"),
        ("join misaligned skip, plain", "ctrl_op_unet_skip_join", join(skip=odd)[:-1], "unet_skip_join: pointers must be 16-byte aligned"),
        ("join C2 = 48", "ctrl_op_unet_skip_join_split", join(C2=48, ld_out=96, lo_off=48), "unet_skip_join: C2 must be a multiple of 32"),
        ("join C2 = 48, plain", "ctrl_op_unet_skip_join", join(C2=48, ld_out=96)[:-1], "unet_skip_join: C2 must be a multiple of 32"),
    ]
    po = lambda lat=4, ldx=8, kind=0, eps=True, out_dt=0: [P(), Q(ldx), I(0), P(), P(), I(1), I(lat), I(2), I(2), P() if eps else null, I(0), F(1.0),
                                                             I(kind), P(), I(out_dt)]
    rows += [
        ("posterior lat = 9", "ctrl_op_vae_posterior", po(lat=9, ldx=18), "vae_posterior: bad shape"),
        ("posterior ldx < 2 lat", "ctrl_op_vae_posterior", po(ldx=7), "vae_posterior: bad shape"),
        ("posterior kind 3", "ctrl_op_vae_posterior", po(kind=3), "vae_posterior: kind must be"),
        ("posterior sample without eps", "ctrl_op_vae_posterior", po(kind=1, eps=False), "vae_posterior: sampling needs eps"),
        ("posterior out dtype 3", "ctrl_op_vae_posterior", po(out_dt=3), "vae_posterior: bad dtype"),
    ]
    hd = lambda lat=4, Cout=16, cs=4, out=None: [P(), I(0), F(1.0), P(), P(), P(), P(), out or P(), I(lat), I(2), I(2), Q(cs), I(Cout)]
    rows += [
        ("head Cout = 24", "ctrl_op_vae_dec_head", hd(Cout=24), "vae_dec_head: bad shape"),
        ("head lat = 9", "ctrl_op_vae_dec_head", hd(lat=9), "vae_dec_head: bad shape"),
        ("head misaligned out", "ctrl_op_vae_dec_head", hd(out=odd), "vae_dec_head: bad shape"),
        ("head channel stride 3", "ctrl_op_vae_dec_head", hd(cs=3), "vae_dec_head: the channel stride"),
    ]
    tl = lambda x=None, C_=32, Cout=3, kind=0, dt=0: [x or P(), P(), P(), P(), F(1e-6), P(), P(), I(2), I(2), I(C_), I(Cout), I(kind), P(), I(dt)]
    rows += [
        ("tail C = 48", "ctrl_op_vae_dec_tail", tl(C_=48), "vae_dec_tail: bad shape"),
        ("tail Cout = 5", "ctrl_op_vae_dec_tail", tl(Cout=5), "vae_dec_tail: bad shape"),
        ("tail misaligned x", "ctrl_op_vae_dec_tail", tl(x=odd), "vae_dec_tail: bad shape"),
        ("tail kind 3", "ctrl_op_vae_dec_tail", tl(kind=3), "vae_dec_tail: kind must be"),
        ("tail dtype 3", "ctrl_op_vae_dec_tail", tl(dt=3), "vae_dec_tail: bad dtype"),
    ]
    tc = lambda Cout=3, kind=0, dt=0, F_=2: [P(), P(), P(), I(F_), I(2), I(2), I(Cout), I(kind), P(), I(dt)]
    rows += [
        ("time conv Cout = 5", "ctrl_op_vae_time_conv", tc(Cout=5), "vae_time_conv: bad shape"),
        ("time conv F = 0", "ctrl_op_vae_time_conv", tc(F_=0), "vae_time_conv: bad shape"),
        ("time conv kind 3", "ctrl_op_vae_time_conv", tc(kind=3), "vae_time_conv: kind must be"),
        ("time conv dtype 3", "ctrl_op_vae_time_conv", tc(dt=3), "vae_time_conv: bad dtype"),
    ]
    en = lambda x=None, F_=3, dt=0, wts=True: [x or P(), P() if wts else null, P(), I(dt), P(), null, I(1), I(F_), I(4), I(0)]
    rows += [
        ("encoder F = 33", "ctrl_op_i2v_latent_encoder", en(F_=33), "i2v_latent_encoder: 1 .. 32 frames"),
        ("encoder no weights", "ctrl_op_i2v_latent_encoder", en(wts=False), "i2v_latent_encoder: null argument"),
        ("encoder sample dtype 3", "ctrl_op_i2v_latent_encoder", en(dt=3), "i2v_latent_encoder: the sample must be"),
        ("encoder misaligned x", "ctrl_op_i2v_latent_encoder", en(x=odd), "i2v_latent_encoder: pointers must be 16-byte aligned"),
        ("avgpool bf16 in", "ctrl_op_adaptive_avgpool_nhwc", [P(), I(2), P(), I(0), I(1), I(2), I(2), I(1), I(2), I(2)], "adaptive_avgpool_nhwc: fp32 or fp16 maps"),
        ("avgpool bf16 out", "ctrl_op_adaptive_avgpool_nhwc", [P(), I(0), P(), I(2), I(1), I(2), I(2), I(1), I(2), I(2)], "adaptive_avgpool_nhwc: fp32 or fp16 maps"),
        ("avgpool OH = 0", "ctrl_op_adaptive_avgpool_nhwc", [P(), I(0), P(), I(0), I(1), I(2), I(2), I(1), I(0), I(2)], "adaptive_avgpool_nhwc: bad arguments"),
        ("text_time odd dim", "ctrl_op_unet_text_time", [P(), I(0), I(4), P(), I(1), I(5), P(), Q(16), I(1)], "unet_text_time: bad sizes"),
        ("text_time narrow rows", "ctrl_op_unet_text_time", [P(), I(0), I(4), P(), I(2), I(6), P(), Q(15), I(1)], "unet_text_time: bad sizes"),
        ("text_time dtype 3", "ctrl_op_unet_text_time", [P(), I(3), I(4), P(), I(1), I(6), P(), Q(16), I(1)], "unet_text_time: text_embeds must be"),
    ]
    return rows
