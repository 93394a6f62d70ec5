"""Thin Python wrappers over the op-level C ABI (ctrl_op_*): allocate outputs with torch, pass raw pointers.

Used by the parity tests and micro-benchmarks; the product forward path goes through the plan-level
entry points (controlnet.py / ctrl_adapter.py) and never composes these from Python.
"""
import ctypes as C

import torch

from . import _lib as L

IG_ROWS, IG_CONV2D, IG_TEMPORAL, IG_CONV2D_PHASE = 0, 1, 2, 3
SEG_ROW, SEG_TRANSPOSED = 0, 1


def _f16(*shape, device="cuda"):
    return torch.empty(*shape, dtype=torch.float16, device=device)


def pack_conv_w(w, ovf=None):
    """[Cout][Cin][kh][kw] -> fp16 [Cout][kh*kw][Cin]"""
    cout, cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    out = _f16(cout, taps * cin)
    if ovf is not None:          # the plans' fp16 range flag (device int32): set to 1, never cleared
        L.check(L.lib().ctrl_op_pack_conv_w_ovf(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, taps, L.ptr(ovf), L.cur_stream()))
        return out
    L.check(L.lib().ctrl_op_pack_conv_w(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, taps, L.cur_stream()))
    return out


def pack_conv_w_dup(w, ovf=None):
    """[Cout][Cin][kh][kw] -> fp16 [Cout][kh*kw][2*Cin] (split-operand convolution: every tap's weights twice)"""
    cout, cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    out = _f16(cout, taps * 2 * cin)
    if ovf is not None:          # the plans' fp16 range flag (device int32): set to 1, never cleared
        L.check(L.lib().ctrl_op_pack_conv_w_dup_ovf(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, taps, L.ptr(ovf), L.cur_stream()))
        return out
    L.check(L.lib().ctrl_op_pack_conv_w_dup(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, taps, L.cur_stream()))
    return out


def pack_conv_w_phase(w, ovf=None):
    """[Cout][Cin][3][3] -> fp16 [4][Cout][4*Cin]: the four 2x2 phase convs of a 3x3 conv over a nearest x2 up-sampled map
    (include/ctrl_hip.h: ctrl_op_pack_conv_w_phase; the W operand of an IG_CONV2D_PHASE problem)"""
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3)
    out = _f16(4, cout, 4 * cin, device=w.device)
    if ovf is not None:          # the plans' fp16 range flag (device int32): set to 1, never cleared
        L.check(L.lib().ctrl_op_pack_conv_w_phase_ovf(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, L.ptr(ovf), L.cur_stream()))
        return out
    L.check(L.lib().ctrl_op_pack_conv_w_phase(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, L.cur_stream()))
    return out


def pack_conv_w_direct(w):
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty(9, cin, cout, dtype=torch.float32, device=w.device)
    L.check(L.lib().ctrl_op_pack_conv_w_direct(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cout, cin, L.cur_stream()))
    return out


def pack_linear_w(w, geglu=False, ovf=None):
    n, k = w.shape
    out = _f16(n, k)
    if ovf is not None:
        L.check(L.lib().ctrl_op_pack_linear_w_ovf(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), n, k, int(geglu), L.ptr(ovf),
                                                  L.cur_stream()))
        return out
    L.check(L.lib().ctrl_op_pack_linear_w(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), n, k, int(geglu), L.cur_stream()))
    return out


def pack_vec(v, geglu=False):
    out = torch.empty(v.numel(), dtype=torch.float32, device=v.device)
    L.check(L.lib().ctrl_op_pack_vec(L.ptr(v.contiguous()), L.dtype_code(v.dtype), L.ptr(out), v.numel(), int(geglu), L.cur_stream()))
    return out


def igemm(A, lda, W, M, Nout, Cin, taps=1, mode=IG_ROWS, geom=None, bias=None, rowvec=None, rows_per_img=1,
          res=None, ldres=0, scale=1.0, geglu=False, segs=None, F=0, HW=0, out16=None, ld16=0, splitk_ws=None,
          blend_mix=None, blend_x=None, ld_blend=0, a_split=False, out16_lo_off=0, t_pad=False, scale2=0.0, scale2_from=0,
          res_up=0, scale2_to=0, tap_origin=0, pinned=False, splitk_tickets=None, act=0):
    """segs: list of (out_tensor, ld, col_begin, ncols, fmt, L); res_up=2: `res` is [N][Hout/2][Wout/2][ldres], read through a
    nearest x2 up-sampling (conv2d); pinned: the encoder plans' fixed 64 x 64 x 64 form (op_igemm_pinned) instead of the dispatcher;
    splitk_tickets: zeroed int32 ticket words of the in-launch split-K reduction (None: the library zeroes its own)"""
    d = igemm_desc(**{k: v for k, v in locals().items() if k != "pinned"})
    L.check((L.lib().ctrl_op_igemm_pinned if pinned else L.lib().ctrl_op_igemm)(C.byref(d), L.cur_stream()))


def igemm_group(descs):
    """1..4 problems (igemm_desc) through ctrl_op_igemm_group: one launch when they agree in everything but their addresses, else one
    launch each; the caller keeps the tensors behind the descriptors alive"""
    arr = (L.IGemmDesc * len(descs))(*descs)
    L.check(L.lib().ctrl_op_igemm_group(arr, len(descs), L.cur_stream()))


def igemm_splitk_plan(d):
    """(splits, scratch bytes, ticket words) ctrl_op_igemm would use for the descriptor `d` (igemm_desc) given a split-K scratch: the
    descriptor must already carry a non-null, aligned splitk_ws (the choice depends on pointer alignment), of any size"""
    lib = L.lib()
    sk = lib.ctrl_igemm_splitk_factor(C.byref(d))
    return sk, int(lib.ctrl_igemm_splitk_ws_bytes(C.byref(d), sk)), int(lib.ctrl_igemm_splitk_ticket_words(C.byref(d), sk))


def igemm_select(d, group_n=1, pinned=False):
    """what ctrl_op_igemm (pinned: ctrl_op_igemm_pinned) would record for the descriptor `d` (igemm_desc) as one of group_n problems of
    a launch: "<kernel symbol>[ splitkN[ in-launch]]".  Launches nothing and needs no GPU."""
    buf = C.create_string_buffer(160)
    L.check(L.lib().ctrl_igemm_select(C.byref(d), int(group_n), int(bool(pinned)), buf, len(buf)))
    return buf.value.decode()


def igemm_desc(A, lda, W, M, Nout, Cin, taps=1, mode=IG_ROWS, geom=None, bias=None, rowvec=None, rows_per_img=1,
               res=None, ldres=0, scale=1.0, geglu=False, segs=None, F=0, HW=0, out16=None, ld16=0, splitk_ws=None,
               blend_mix=None, blend_x=None, ld_blend=0, a_split=False, out16_lo_off=0, t_pad=False, scale2=0.0, scale2_from=0,
               res_up=0, scale2_to=0, tap_origin=0, splitk_tickets=None, act=0):
    """the ctrl_igemm_desc of ops.igemm's arguments (the tensors must stay alive while it is used)"""
    d = L.IGemmDesc()
    d.A = A.data_ptr(); d.lda = lda; d.mode = mode; d.Cin = Cin; d.taps = taps
    g = geom or {}
    d.Hin = g.get("Hin", 1); d.Win = g.get("Win", 1); d.Hout = g.get("Hout", 1); d.Wout = g.get("Wout", 1)
    d.stride = g.get("stride", 1); d.up = g.get("up", 1); d.tap_origin = tap_origin
    d.F = F; d.HW = HW; d.t_pad = int(t_pad)
    d.W = W.data_ptr(); d.M = M; d.Nout = Nout; d.Ktot = taps * Cin
    d.bias = bias.data_ptr() if bias is not None else None
    d.rowvec = rowvec.data_ptr() if rowvec is not None else None
    d.rowvec_ld = rowvec.shape[-1] if rowvec is not None else 0
    d.rows_per_img = rows_per_img
    d.res = res.data_ptr() if res is not None else None
    d.ldres = ldres
    d.res_f32 = int(res is not None and res.dtype == torch.float32)
    d.res_up = res_up
    d.out16 = out16.data_ptr() if out16 is not None else None
    d.splitk_ws = splitk_ws.data_ptr() if splitk_ws is not None else None
    d.splitk_ws_bytes = splitk_ws.numel() * splitk_ws.element_size() if splitk_ws is not None else 0
    d.splitk_tickets = splitk_tickets.data_ptr() if splitk_tickets is not None else None
    d.ld16 = ld16
    d.blend_mix = blend_mix.data_ptr() if blend_mix is not None else None
    d.blend_x = blend_x.data_ptr() if blend_x is not None else None
    d.ld_blend = ld_blend
    d.blend_f32 = int(blend_x is not None and blend_x.dtype == torch.float32)
    d.scale = scale; d.geglu = int(geglu); d.act = int(act)      # act: 0 none, 1 SiLU, 2 quick_gelu, 3 ReLU
    d.scale2 = scale2; d.scale2_from = scale2_from; d.scale2_to = scale2_to
    d.a_split = int(a_split); d.out16_lo_off = out16_lo_off      # a_split: 0 | 1 (weights packed twice) | 2 (paired walk)
    d.nseg = len(segs)
    for i, (out, ld, cb, nc, fmt, Ltok) in enumerate(segs):
        d.seg[i].out = out.data_ptr(); d.seg[i].ld = ld; d.seg[i].col_begin = cb; d.seg[i].ncols = nc
        d.seg[i].fmt = fmt; d.seg[i].dtype = L.dtype_code(out.dtype); d.seg[i].L = Ltok
    return d


def ffn_pack_w2(w2_packed):
    """fp16 [512][2048] linear pack of ff.net.2 -> the layout / k order of the fused feed-forward kernel (csrc/ffn.hip)"""
    N, K = w2_packed.shape
    out = torch.empty_like(w2_packed)
    L.check(L.lib().ctrl_op_ffn_pack_w2(L.ptr(w2_packed), L.ptr(out), N, K, L.cur_stream()))
    return out


def ffn_desc(x, w1p, b1p, w2pp, out, b2=None, res=None, out16=None, ld=512, ldres=512, ld16=512, blend_mix=None, blend_x=None, ld_blend=512,
             M=None):
    """the ctrl_ffn_desc of ffn_fused's arguments (the tensors must stay alive while it is used).  x, out, res, out16 and blend_x may be
    views into larger buffers: each is addressed from its first element with the row stride given beside it (ld / ldres / ld16 /
    ld_blend in elements; x rows are always 512 apart)"""
    d = L.FfnDesc()
    d.X = x.data_ptr(); d.ldx = x.shape[1]; d.W1 = w1p.data_ptr(); d.b1 = b1p.data_ptr(); d.W2p = w2pp.data_ptr()
    o = d.out
    o.M = x.shape[0] if M is None else M; o.Nout = 512; o.Ktot = 2048; o.Cin = 2048; o.taps = 1; o.scale = 1.0; o.rows_per_img = 1
    o.Hin = o.Win = o.Hout = o.Wout = o.stride = o.up = 1
    o.bias = b2.data_ptr() if b2 is not None else None
    o.res = res.data_ptr() if res is not None else None
    o.ldres = ldres
    o.res_f32 = int(res is not None and res.dtype == torch.float32)
    o.out16 = out16.data_ptr() if out16 is not None else None
    o.ld16 = ld16
    o.blend_mix = blend_mix.data_ptr() if blend_mix is not None else None
    o.blend_x = blend_x.data_ptr() if blend_x is not None else None
    o.ld_blend = ld_blend
    o.blend_f32 = int(blend_x is not None and blend_x.dtype == torch.float32)
    o.nseg = 1
    o.seg[0].out = out.data_ptr(); o.seg[0].ld = ld; o.seg[0].col_begin = 0; o.seg[0].ncols = 512
    o.seg[0].fmt = SEG_ROW; o.seg[0].dtype = L.dtype_code(out.dtype); o.seg[0].L = 1
    return d


def ffn_group(descs):
    """1..4 feed-forwards of equal M (ffn_desc) through ctrl_op_ffn_group: ONE launch, the way the plans launch the sibling adapter
    blocks of a pyramid level; the caller keeps the tensors behind the descriptors alive"""
    arr = (L.FfnDesc * len(descs))(*descs)
    L.check(L.lib().ctrl_op_ffn_group(arr, len(descs), L.cur_stream()))


def ffn_fused(x, w1p, b1p, w2pp, b2=None, res=None, out=None, out16=None, ld=512, ldres=512, ld16=512):
    """out = res + ((x W1h^T + b1h) * gelu(x W1g^T + b1g)) W2^T + b2 in ONE launch (csrc/ffn.hip): x fp16 [M][512]; w1p / b1p the GEGLU
    packs of ff.net.0.proj (pack_linear_w / pack_vec with geglu=True), w2pp = ffn_pack_w2(pack_linear_w(W2)); res fp32 or fp16 [M][512];
    out fp32 or fp16 [M][512] (default fp16), out16 an optional fp16 mirror of an fp32 out; ld / ldres / ld16: the row strides of out /
    res / out16 in elements (views into wider buffers)"""
    if out is None:
        out = _f16(x.shape[0], 512)
    d = ffn_desc(x, w1p, b1p, w2pp, out, b2=b2, res=res, out16=out16, ld=ld, ldres=ldres, ld16=ld16)
    L.check(L.lib().ctrl_op_ffn(C.byref(d), L.cur_stream()))
    return out


def set_igemm_order(spec):
    """tile walk of the implicit GEMM over the XCDs: "auto" (default) | "legacy" | "m,G" | "n,G" (csrc/tile_order.h); results
    do not depend on it"""
    if L.lib().ctrl_igemm_set_order(spec.encode()) != 0:
        raise ValueError("unknown tile walk order %r" % (spec,))


def set_igemm_wide(mode):
    """which GEMM / convolution problems run on the 8-phase wide-tile kernel: 0 none, 1 where the grid fills the chip (default), 2 every
    eligible problem (tests), -1 back to the default (csrc/igemm.hip)"""
    L.check(L.lib().ctrl_igemm_set_wide(int(mode)))


def set_group_launches(mode):
    """grouped launches over the sibling adapter blocks of a pyramid level (csrc/ops.h: OpCollector): 1 / True on (default), 2 on with
    the tile selection every problem would get alone (bit-identical to the one-by-one forward), 0 / False off, None queries; returns
    the mode."""
    return int(L.lib().ctrl_group_launches(-1 if mode is None else int(mode)))


def set_policy(name, value):
    """overrides one CTRL_* variable of the library's policy table for this process (csrc/policy.h; value None = unset, as if the
    variable were absent from the environment); returns the previous value (None = unset).  Test / experiment hook."""
    prev = L.lib().ctrl_policy_get(name.encode())
    L.check(L.lib().ctrl_policy_set(name.encode(), None if value is None else str(value).encode()))
    return None if prev is None else prev.decode()


def policy():
    """{name: value} of every CTRL_* variable that is set (environment snapshot + overrides)"""
    lib = L.lib()
    out = {}
    for i in range(lib.ctrl_policy_count()):
        n = lib.ctrl_policy_name(i)
        v = lib.ctrl_policy_get(n)
        if v is not None:
            out[n.decode()] = v.decode()
    return out


def set_attn_variant(v):
    """instruction-selection variant of the head_dim-64 long-sequence attention kernel (0 = the round-2 kernel); every
    variant computes the same function (csrc/attention_d64.hip)"""
    L.check(L.lib().ctrl_attn_set_variant(int(v)))


def linear(x, w_packed, bias=None, res=None, geglu=False):
    """x [M][K] fp16 -> [M][N] fp16 (N/2 for GEGLU)"""
    M, K = x.shape
    N = w_packed.shape[0]
    on = N // 2 if geglu else N
    out = _f16(M, on)
    igemm(x, K, w_packed, M, N, K, bias=bias, res=res, ldres=on, geglu=geglu,
          segs=[(out, on, 0, on, SEG_ROW, 1)])
    return out


def conv2d(x_nhwc, w_packed, Cout, taps=9, stride=1, up=1, bias=None, rowvec=None, res=None, scale=1.0,
           out_nchw_dtype=None, splitk_ws=None, res_up=0):
    """x [N][H][W][Cin] fp16 -> [N][Ho][Wo][Cout] fp16 (or NCHW in out_nchw_dtype)"""
    N, H, W, Cin = x_nhwc.shape
    pad = 1 if taps == 9 else 0
    Ho = (H * up + 2 * pad - (3 if taps == 9 else 1)) // stride + 1
    Wo = (W * up + 2 * pad - (3 if taps == 9 else 1)) // stride + 1
    M = N * Ho * Wo
    geom = dict(Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=stride, up=up)
    if out_nchw_dtype is None:
        out = _f16(N, Ho, Wo, Cout)
        segs = [(out, Cout, 0, Cout, SEG_ROW, 1)]
    else:
        out = torch.empty(N, Cout, Ho, Wo, dtype=out_nchw_dtype, device=x_nhwc.device)
        segs = [(out, Ho * Wo, 0, Cout, SEG_TRANSPOSED, Ho * Wo)]
    igemm(x_nhwc, Cin, w_packed, M, Cout, Cin, taps=taps, mode=IG_CONV2D, geom=geom, bias=bias, rowvec=rowvec,
          rows_per_img=Ho * Wo, res=res, ldres=Cout, scale=scale, segs=segs, splitk_ws=splitk_ws, res_up=res_up)
    return out


def flash_attn_desc(Q, ldq, K, ldk, Vt, Lkpad, B, heads, D, Lq, Lk, out, ldo, scale=None, kvB=0, k_prescaled=False):
    """the ctrl_attn_desc of one problem.  Q, K, Vt and out may be views into larger buffers: each is addressed from its first element
    (data_ptr) with the leading dimension given beside it (ldq / ldk / ldo in elements; Vt rows are Lkpad apart)."""
    d = L.AttnDesc()
    d.Q = Q.data_ptr(); d.ldq = ldq; d.K = K.data_ptr(); d.ldk = ldk; d.Vt = Vt.data_ptr(); d.Lkpad = Lkpad
    d.O = out.data_ptr(); d.ldo = ldo
    d.B = B; d.heads = heads; d.D = D; d.Lq = Lq; d.Lk = Lk; d.kvB = kvB if kvB else B
    d.scale = scale if scale is not None else D ** -0.5
    d.k_prescaled = int(k_prescaled)
    return d


def flash_attn(Q, ldq, K, ldk, Vt, Lkpad, B, heads, D, Lq, Lk, scale=None, kvB=0, k_prescaled=False, out=None, ldo=None):
    """-> [B*Lq][heads*D] fp16 (dense), or written into `out` (a view whose rows are `ldo` elements apart; default: its row stride)"""
    if out is None:
        out = _f16(B * Lq, heads * D)
        ldo = heads * D
    elif ldo is None:
        ldo = out.stride(0)
    d = flash_attn_desc(Q, ldq, K, ldk, Vt, Lkpad, B, heads, D, Lq, Lk, out, ldo, scale=scale, kvB=kvB, k_prescaled=k_prescaled)
    L.check(L.lib().ctrl_op_flash_attn(C.byref(d), L.cur_stream()))
    return out


def flash_attn_group(descs):
    """1..4 problems (flash_attn_desc) through ctrl_op_flash_attn_group: one launch when they agree in shape, strides and pointer
    phase, else one launch each; the caller keeps the tensors behind the descriptors alive"""
    arr = (L.AttnDesc * len(descs))(*descs)
    L.check(L.lib().ctrl_op_flash_attn_group(arr, len(descs), L.cur_stream()))


def temporal_attn(qkv, Bc, F, HW, heads, kv=None, Fq=0, Fl=0, out=None, ldo=None):
    """qkv [(b f) p][3C] (q | k | v) -> [(b f) p][C]; sharded form: qkv holds the LOCAL Fq query frames as [..][C] rows
    and kv = the gathered K|V rows [world][Bc][Fl][HW][2C].  qkv may be a view (its row stride is the leading dimension); `out`:
    a view to write into, rows `ldo` elements apart (default: its row stride)"""
    Cc = heads * 64
    if out is None:
        out = _f16(qkv.shape[0], Cc)
        ldo = Cc
    elif ldo is None:
        ldo = out.stride(0)
    d = L.TAttnDesc()
    d.Q = qkv.data_ptr(); d.ld = qkv.stride(0); d.O = out.data_ptr(); d.ldo = ldo
    d.Bc = Bc; d.F = F; d.HW = HW; d.heads = heads; d.scale = 64 ** -0.5
    d.Fq = Fq; d.Fl = Fl
    if kv is not None:
        d.KV = kv.data_ptr(); d.ldkv = kv.shape[-1]
    L.check(L.lib().ctrl_op_temporal_attn(C.byref(d), L.cur_stream()))
    return out


def groupnorm(x, gamma, beta, imgs, rows_per_img, G=32, eps=1e-5, silu=False):
    Cc = x.shape[-1]
    lib = L.lib()
    stats = torch.zeros(lib.ctrl_op_gn_stats_floats(imgs, rows_per_img, Cc, G), dtype=torch.float32, device=x.device)
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    L.check(lib.ctrl_op_gn_stats(L.ptr(x), L.dtype_code(x.dtype), L.ptr(stats), imgs, rows_per_img, Cc, G, L.cur_stream()))
    L.check(lib.ctrl_op_gn_apply(L.ptr(x), L.dtype_code(x.dtype), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(y), imgs, rows_per_img, Cc, G,
                                 C.c_float(eps), int(silu), L.cur_stream()))
    return y


def groupnorm_fused(x, gamma, beta, imgs, rows_per_img, G=32, eps=1e-5, silu=False, split=False):
    """GroupNorm(32) of a small map in one launch (csrc/norm.hip: gn_fused_kernel); None when the problem does not qualify"""
    Cc = x.shape[-1]
    lib = L.lib()
    if not lib.ctrl_op_gn_fused_applies(L.dtype_code(x.dtype), rows_per_img, Cc, G):
        return None
    y = torch.empty(tuple(x.shape[:-1]) + ((2 * Cc) if split else Cc,), dtype=torch.float16, device=x.device)
    L.check(lib.ctrl_op_gn_fused(L.ptr(x), L.dtype_code(x.dtype), L.ptr(gamma), L.ptr(beta), L.ptr(y), C.c_int64(2 * Cc if split else Cc),
                                 Cc if split else 0, imgs, rows_per_img, Cc, G, C.c_float(eps), int(silu), L.cur_stream()))
    return y


def groupnorm_split(x, gamma, beta, imgs, rows_per_img, G=32, eps=1e-5, silu=False):
    """GroupNorm whose result is a split operand: [rows][2C] = [hi | lo], hi + lo == the fp32 result to ~2^-22"""
    Cc = x.shape[-1]
    lib = L.lib()
    stats = torch.zeros(lib.ctrl_op_gn_stats_floats(imgs, rows_per_img, Cc, G), dtype=torch.float32, device=x.device)
    y = torch.empty(tuple(x.shape[:-1]) + (2 * Cc,), dtype=torch.float16, device=x.device)
    L.check(lib.ctrl_op_gn_stats(L.ptr(x), L.dtype_code(x.dtype), L.ptr(stats), imgs, rows_per_img, Cc, G, L.cur_stream()))
    L.check(lib.ctrl_op_gn_apply_split(L.ptr(x), L.dtype_code(x.dtype), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(y),
                                       C.c_int64(2 * Cc), Cc, imgs, rows_per_img, Cc, G, C.c_float(eps), int(silu), L.cur_stream()))
    return y


def layernorm(x, gamma, beta, eps=1e-5):
    M, Cc = x.shape
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    L.check(L.lib().ctrl_op_layernorm(L.ptr(x), L.dtype_code(x.dtype), C.c_int64(Cc), L.ptr(gamma), L.ptr(beta), L.ptr(y), C.c_int64(Cc), M, Cc,
                                      C.c_float(eps), L.cur_stream()))
    return y


# ---- the test ABI of the norm and streaming kernels (tests/norm_forms.py, tests/test_gpu_stream_forms.py): thin, every argument ----
def gn_desc(x, imgs, rows_per_img, Cc, G, stats=None, gamma=None, beta=None, y=None, eps=1e-5, silu=False, ldx=0, ldy=0, lo_off=0,
            stat_rows=0, y_img_rows=0, y_row0=0):
    """ctrl_gn_desc over views the caller keeps alive (x may be a column range of wider rows: pass its row stride as ldx)"""
    d = L.GnDesc()
    d.x = x.data_ptr(); d.x_dtype = L.dtype_code(x.dtype); d.silu = int(silu)
    d.stats = stats.data_ptr() if stats is not None else 0
    d.gamma = gamma.data_ptr() if gamma is not None else 0
    d.beta = beta.data_ptr() if beta is not None else 0
    d.y = y.data_ptr() if y is not None else 0
    d.imgs = imgs; d.rows_per_img = rows_per_img; d.C = Cc; d.G = G; d.eps = eps; d.lo_off = lo_off
    d.ldx = ldx; d.ldy = ldy; d.stat_rows = stat_rows; d.y_img_rows = y_img_rows; d.y_row0 = y_row0
    return d


def _group(fn, cls, descs):
    arr = (cls * len(descs))(*descs)
    L.check(fn(arr, len(descs), L.cur_stream()))


def gn_stats_group(descs):
    _group(L.lib().ctrl_op_gn_stats_group, L.GnDesc, descs)


def gn_apply_group(descs):
    _group(L.lib().ctrl_op_gn_apply_group, L.GnDesc, descs)


def gn_fused_group(descs):
    _group(L.lib().ctrl_op_gn_fused_group, L.GnDesc, descs)


def gn_stats_floats(imgs, rows_per_img, Cc, G):
    return int(L.lib().ctrl_op_gn_stats_floats(imgs, rows_per_img, Cc, G))


def gn_launch_shape(imgs, rows_per_img, Cc, which):
    """(rows_per_block, chunks) of the statistics (which = 0) / apply (1) launch, as the launchers compute them; host only"""
    rpb, chunks = C.c_int(), C.c_int()
    L.check(L.lib().ctrl_gn_launch_shape(imgs, rows_per_img, Cc, which, C.byref(rpb), C.byref(chunks)))
    return rpb.value, chunks.value


def ln_desc(x, gamma, beta, y, M, Cc, ldx, ldy, eps=1e-5, addv=None, ldv=0, rows_per_img=0, vmod=0, xsum=None):
    d = L.LnDesc()
    d.x = x.data_ptr(); d.x_dtype = L.dtype_code(x.dtype); d.M = M; d.ldx = ldx
    d.addv = addv.data_ptr() if addv is not None else 0
    d.ldv = ldv; d.rows_per_img = rows_per_img; d.vmod = vmod
    d.xsum = xsum.data_ptr() if xsum is not None else 0
    d.gamma = gamma.data_ptr(); d.beta = beta.data_ptr(); d.y = y.data_ptr(); d.ldy = ldy; d.C = Cc; d.eps = eps
    return d


def layernorm_group(descs):
    _group(L.lib().ctrl_op_layernorm_group, L.LnDesc, descs)


def layernorm_add(x, addv, ldv, rows_per_img, vmod, xsum, gamma, beta, y, M, Cc, ldx, ldy, eps=1e-5):
    """xsum = x + addv[(row / rows_per_img) % vmod] (x's dtype, row stride ldx), y = LayerNorm(xsum)"""
    L.check(L.lib().ctrl_op_layernorm_add(L.ptr(x), L.dtype_code(x.dtype), ldx, L.ptr(addv), ldv, rows_per_img, vmod, L.ptr(xsum), L.ptr(gamma),
                                          L.ptr(beta), L.ptr(y), ldy, M, Cc, eps, L.cur_stream()))


def add_rowvec_clip(x, v, ldv, y, B, F, Lp, Cc):
    """y[(b f p)] = x + v[(b * Lp + p) % B]; y may be x (in place)"""
    L.check(L.lib().ctrl_op_add_rowvec_clip(L.ptr(x), L.dtype_code(x.dtype), L.ptr(v), ldv, L.ptr(y), L.dtype_code(y.dtype), B, F, Lp, Cc,
                                            L.cur_stream()))


def upsample2x_nhwc(x):
    N, H, W, Cc = x.shape
    y = _f16(N, 2 * H, 2 * W, Cc)
    L.check(L.lib().ctrl_op_upsample2x_nhwc(L.ptr(x), L.ptr(y), N, H, W, Cc, L.cur_stream()))
    return y


def fill_zero_group(ptrs, sizes):
    """zero sizes[i] bytes at device address ptrs[i], 1..4 fills in one launch"""
    n = len(ptrs)
    pa = (C.c_void_p * n)(*ptrs)
    sa = (C.c_size_t * n)(*sizes)
    L.check(L.lib().ctrl_op_fill_zero_group(pa, sa, n, L.cur_stream()))


def small_lin(x, ldx, w, b, out, ldo, M, N, K, in_silu=False, out_silu=False):
    d = L.SmallLin()
    d.x = x.data_ptr(); d.ldx = ldx; d.w = w.data_ptr(); d.b = b.data_ptr() if b is not None else 0
    d.out = out.data_ptr(); d.ldo = ldo; d.M = M; d.N = N; d.K = K; d.in_silu = int(in_silu); d.out_silu = int(out_silu)
    return d


def linear_small_group(descs):
    _group(L.lib().ctrl_op_linear_small_group, L.SmallLin, descs)


def linear_small_into(x, ldx, w, b, out, ldo, M, N, K, in_silu=False, out_silu=False):
    L.check(L.lib().ctrl_op_linear_small(L.ptr(x), ldx, L.ptr(w), L.ptr(b), L.ptr(out), ldo, M, N, K, int(in_silu), int(out_silu),
                                         L.cur_stream()))


def frameidx_sincos(N, F, dim, device="cuda"):
    out = torch.empty(N, dim, dtype=torch.float32, device=device)
    L.check(L.lib().ctrl_op_frameidx_sincos(L.ptr(out), N, F, dim, L.cur_stream()))
    return out


def nchw_to_nhwc(x):
    N, Cc, H, W = x.shape
    y = _f16(N, H, W, Cc)
    L.check(L.lib().ctrl_op_nchw_to_nhwc(L.ptr(x.contiguous()), L.dtype_code(x.dtype), L.ptr(y), N, Cc, H * W, L.cur_stream()))
    return y


def nhwc_to_nchw(x, dtype=torch.float32, scale=1.0):
    N, H, W, Cc = x.shape
    y = torch.empty(N, Cc, H, W, dtype=dtype, device=x.device)
    L.check(L.lib().ctrl_op_nhwc_to_nchw(L.ptr(x), L.ptr(y), L.dtype_code(dtype), N, Cc, H * W, C.c_float(scale), L.cur_stream()))
    return y


def avgpool_nchw(x, Hout, Wout):
    """exact integer-ratio F.adaptive_avg_pool2d; dtype preserved"""
    N, Cc, H, W = x.shape
    y = torch.empty(N, Cc, Hout, Wout, dtype=x.dtype, device=x.device)
    L.check(L.lib().ctrl_avgpool_nchw(L.ptr(x.contiguous()), L.ptr(y), L.dtype_code(x.dtype), N * Cc, H, W, Hout, Wout, L.cur_stream()))
    return y


def timestep_sincos(t, N, dim):
    out = torch.empty(N, dim, dtype=torch.float32, device=t.device)
    L.check(L.lib().ctrl_op_timestep_sincos(L.ptr(t), t.numel(), L.ptr(out), N, dim, L.cur_stream()))
    return out


def linear_small(x, w_packed, bias=None, in_silu=False, out_silu=False):
    M, K = x.shape
    N = w_packed.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    L.check(L.lib().ctrl_op_linear_small(L.ptr(x), C.c_int64(K), L.ptr(w_packed), L.ptr(bias), L.ptr(out), C.c_int64(N), M, N, K,
                                         int(in_silu), int(out_silu), L.cur_stream()))
    return out


def blend(xs, xt, mix):
    y = torch.empty_like(xs)
    L.check(L.lib().ctrl_op_blend(L.ptr(xs), L.dtype_code(xs.dtype), L.ptr(xt), L.dtype_code(xt.dtype), L.ptr(mix), L.ptr(y),
                                  L.dtype_code(y.dtype), C.c_size_t(xs.numel()), L.cur_stream()))
    return y


def add_rowvec(x, v, rows_per_img, vmod):
    M, Cc = x.shape
    y = torch.empty_like(x)
    L.check(L.lib().ctrl_op_add_rowvec(L.ptr(x), L.dtype_code(x.dtype), L.ptr(v), C.c_int64(v.shape[-1]), L.ptr(y), L.dtype_code(y.dtype),
                                       C.c_size_t(M), Cc, rows_per_img, vmod, L.cur_stream()))
    return y


def blend_into(xs, xt, mix, y, n=None):
    """y = sigmoid(mix) xs + (1 - sigmoid(mix)) xt over the first n elements (default: all of xs); xs, xt, y fp16 or fp32, each its own"""
    L.check(L.lib().ctrl_op_blend(L.ptr(xs), L.dtype_code(xs.dtype), L.ptr(xt), L.dtype_code(xt.dtype), L.ptr(mix), L.ptr(y),
                                  L.dtype_code(y.dtype), C.c_size_t(xs.numel() if n is None else n), L.cur_stream()))


def add_rowvec_into(x, v, ldv, y, M, Cc, rows_per_img, vmod):
    """y[m] = x[m] + v[(m // rows_per_img) % vmod] over M dense rows of Cc; v rows ldv apart; y may be x, and of another dtype"""
    L.check(L.lib().ctrl_op_add_rowvec(L.ptr(x), L.dtype_code(x.dtype), L.ptr(v), C.c_int64(ldv), L.ptr(y), L.dtype_code(y.dtype),
                                       C.c_size_t(M), Cc, rows_per_img, vmod, L.cur_stream()))


def nhwc_to_nchw_into(x, y, N, Cc, HW, scale=1.0, img_map=None):
    """fp16 [N][HW][Cc] -> y [..][Cc][HW] * scale in y's dtype; img_map (int32 device [N]): source image n lands at image img_map[n]"""
    L.check(L.lib().ctrl_op_nhwc_to_nchw_map(L.ptr(x), L.ptr(y), L.dtype_code(y.dtype), N, Cc, HW, C.c_float(scale), L.ptr(img_map),
                                             L.cur_stream()))


CONV_OUT_NCHW, CONV_OUT_NCFHW, CONV_OUT_ROWS = 0, 1, 2


def unet_conv_out(x, w_direct, bias, out, N, H, W, Cc, Cout, layout=CONV_OUT_NCHW, frames=1):
    """the backbone UNets' conv_out: x fp16 [N][H][W][Cc], w_direct = pack_conv_w_direct(w) -> out in its dtype and `layout`"""
    L.check(L.lib().ctrl_op_unet_conv_out(L.ptr(x), L.ptr(w_direct), L.ptr(bias), L.ptr(out), L.dtype_code(out.dtype), N, H, W, Cc, Cout,
                                          layout, frames, L.cur_stream()))


def i2v_frames(x, y, B, F, HW):
    """[B][4][F][HW] of any dtype -> fp32 [(b f)][4][HW]"""
    L.check(L.lib().ctrl_op_i2v_frames(L.ptr(x), L.dtype_code(x.dtype), L.ptr(y), B, F, HW, L.cur_stream()))


def vae_conv_in(px, w_direct, bias, out, H, W, Cout):
    """the KL-VAE encoder's conv_in of one image: NCHW pixels [3][H][W] -> fp32 rows [H*W][Cout]"""
    L.check(L.lib().ctrl_op_vae_conv_in(L.ptr(px), L.dtype_code(px.dtype), L.ptr(w_direct), L.ptr(bias), L.ptr(out), H, W, Cout,
                                        L.cur_stream()))


def vae_row_softmax(S, lds, P, ldp, rows, Lr, Lpad):
    """P[r][:Lr] = softmax(S[r][:Lr]) in fp16, P[r][Lr:Lpad] = 0; rows lds / ldp apart"""
    L.check(L.lib().ctrl_op_vae_row_softmax(L.ptr(S), lds, L.ptr(P), ldp, rows, Lr, Lpad, L.cur_stream()))


def conv3x3_direct(x, w_direct, bias, Cout, stride=1, silu=False, nchw=False, out=None):
    """x NCHW of any dtype (Cin 3 | 4) or NHWC fp16 (Cin 16 | 32), w_direct = pack_conv_w_direct(w) -> fp16 NHWC [N][Ho][Wo][Cout]
    (`out`: a dense fp16 tensor of that size to write into)"""
    if nchw:
        N, Cin, H, W = x.shape
    else:
        N, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = _f16(N, Ho, Wo, Cout)
    L.check(L.lib().ctrl_op_conv3x3_direct(L.ptr(x), L.dtype_code(x.dtype), int(nchw), L.ptr(w_direct), L.ptr(bias), L.ptr(out),
                                           N, Cin, Cout, H, W, stride, int(silu), L.cur_stream()))
    return out


def conv3x3_direct_f32(x_nchw, w_direct, bias, Cout, out=None):
    """the backbone UNets' stem: x NCHW [N][Cin][H][W] of any dtype (Cin 4 | 8) -> fp32 rows [N][H][W][Cout] (stride 1, no activation)"""
    N, Cin, H, W = x_nchw.shape
    if out is None:
        out = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x_nchw.device)
    L.check(L.lib().ctrl_op_conv3x3_direct_f32(L.ptr(x_nchw), L.dtype_code(x_nchw.dtype), L.ptr(w_direct), L.ptr(bias), L.ptr(out), N, Cin, Cout,
                                               H, W, L.cur_stream()))
    return out


def conv3x3_rows_f32(x_rows, w_direct, bias, Cout, out=None):
    """the I2VGen-XL UNet's stem: x fp32 channels-last [N][H][W][8] -> fp32 rows [N][H][W][Cout] (stride 1, no activation)"""
    N, H, W, Cin = x_rows.shape
    if out is None:
        out = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x_rows.device)
    L.check(L.lib().ctrl_op_conv3x3_rows_f32(L.ptr(x_rows), L.ptr(w_direct), L.ptr(bias), L.ptr(out), N, Cin, Cout, H, W, L.cur_stream()))
    return out


def conv3x3_small_mfma(x, w_packed, bias, Cout, stride=1, silu=False, out=None):
    """x NHWC fp16 [N][H][W][Cin] (Cin, Cout in {16, 32}), w_packed = pack_conv_w(w): the MFMA form of the small convolutions"""
    N, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = _f16(N, Ho, Wo, Cout)
    L.check(L.lib().ctrl_op_conv3x3_small_mfma(L.ptr(x), L.ptr(w_packed), L.ptr(bias), L.ptr(out), N, Cin, Cout, H, W, stride, int(silu),
                                               L.cur_stream()))
    return out


def router_weights(wg, mask, equal_weights=False):
    R, E = wg.shape
    out = torch.empty(R, E, dtype=torch.float32, device=wg.device)
    m = (C.c_int * E)(*[int(v) for v in mask]) if mask is not None else None
    L.check(L.lib().ctrl_router_weights(L.ptr(wg), m, L.ptr(out), R, E, int(equal_weights), L.cur_stream()))
    return out


def router_merge(experts, weights_row, widx):
    K = len(experts)
    out = torch.empty_like(experts[0])
    ptrs = (C.c_void_p * K)(*[e.data_ptr() for e in experts])
    idx = (C.c_int * K)(*widx)
    L.check(L.lib().ctrl_router_merge(ptrs, L.ptr(weights_row), idx, K, L.ptr(out), L.dtype_code(out.dtype),
                                      C.c_size_t(out.numel()), L.cur_stream()))
    return out


def _merge_gather_args(slots, outs, weights, rows, widx, frame_map, n_in):
    """the C argument list shared by ctrl_op_merge_gather_group and its launch-shape query (everything but the stream / the results)"""
    n = len(slots)
    if not 1 <= n <= L.MERGE_SLOTS or len(outs) != n:
        raise ValueError("merge_gather: 1..%d slots, one output each (got %d slots, %d outputs)" % (L.MERGE_SLOTS, n, len(outs)))
    K = len(slots[0])
    if not 1 <= K <= 8 or any(len(s) != K for s in slots):
        raise ValueError("merge_gather: every slot needs the same 1..8 experts")
    tab = (L.MergeSlot * n)()
    n_out = outs[0].shape[0]
    for i, (xs, o) in enumerate(zip(slots, outs)):
        x0 = xs[0]
        for x in xs:
            if not x.is_cuda or not x.is_contiguous() or x.shape != x0.shape or x.dtype != slots[0][0].dtype or x.shape[0] != n_in:
                raise ValueError("merge_gather: slot %d needs dense GPU experts of one shape [%d, ...] and one dtype" % (i, n_in))
        if not o.is_contiguous() or o.shape[0] != n_out or tuple(o.shape[1:]) != tuple(x0.shape[1:]) or o.dtype != outs[0].dtype:
            raise ValueError("merge_gather: output %d must be a dense [%d, %s] tensor" % (i, n_out, ", ".join(map(str, x0.shape[1:]))))
        for k, x in enumerate(xs):
            tab[i].inp[k] = x.data_ptr()
        tab[i].out, tab[i].elems, tab[i].row = o.data_ptr(), x0[0].numel(), int(rows[i]) if rows is not None else 0
    if frame_map is not None and (frame_map.dtype != torch.int32 or not frame_map.is_cuda or not frame_map.is_contiguous()
                                  or frame_map.numel() != n_out):
        raise ValueError("merge_gather: the map must be a dense int32 GPU tensor of %d frame indices" % n_out)
    if weights is not None and (weights.dim() != 2 or weights.dtype != torch.float32 or not weights.is_cuda or not weights.is_contiguous()):
        raise ValueError("merge_gather: the weights must be a dense fp32 GPU tensor [R, E]")
    R, E = (weights.shape[0], weights.shape[1]) if weights is not None else (0, 0)
    idx = (C.c_int * K)(*[int(v) for v in widx]) if widx is not None else None
    return [tab, n, L.ptr(weights), R, E, idx, K, L.ptr(frame_map), n_in, n_out, L.dtype_code(slots[0][0].dtype), L.dtype_code(outs[0].dtype)]


def merge_gather(slots, weights=None, rows=None, widx=None, frame_map=None, out_dtype=None, out=None):
    """Router merge + key-frame gather + cast of up to 13 slots in one launch (ctrl_op_merge_gather_group).

    slots: a list of slots, each the list of its K expert tensors [n_in, ...] (one dtype, one K for all).  weights: fp32 [R, E] (the
    router's output; None: weight 1, K == 1, an exact gather); rows[s]: the weight row of slot s; widx[k]: the column expert k reads.
    frame_map: int32 device tensor [n_out] of input-frame indices (None: the identity).  Returns the list of [n_out, ...] tensors in
    out_dtype (default: the input dtype).  The host reads no device memory: the call records into a graph."""
    x0 = slots[0][0]
    n_in = x0.shape[0]
    n_out = int(frame_map.numel()) if frame_map is not None else n_in
    odt = out_dtype if out_dtype is not None else x0.dtype
    if out is None:
        out = [torch.empty((n_out,) + tuple(xs[0].shape[1:]), dtype=odt, device=x0.device) for xs in slots]
    args = _merge_gather_args(slots, out, weights, rows, widx, frame_map, n_in)
    with torch.cuda.device(x0.device):
        L.check(L.lib().ctrl_op_merge_gather_group(*args, L.cur_stream()))
    return out


def merge_gather_launch_shape(slots, outs, weights=None, rows=None, widx=None, frame_map=None):
    """(workgroups, elements per thread and access, grid cap) of the merge_gather launch over these tensors (host only)"""
    b, v, cap = C.c_int(), C.c_int(), C.c_int()
    args = _merge_gather_args(slots, outs, weights, rows, widx, frame_map, slots[0][0].shape[0])
    L.check(L.lib().ctrl_op_merge_gather_launch_shape(*args, C.byref(b), C.byref(v), C.byref(cap)))
    return b.value, v.value, cap.value


# ---- the lineart annotator's kernels (csrc/lineart.hip; include/ctrl_hip.h: ctrl_op_lineart_*, ctrl_op_in_*) ----
def pack_convT_w_phase(w, ovf=None):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) weight [Cin][Cout][3][3] -> fp16 [4][Cout][4*Cin]: the W operand of an
    IG_CONV2D_PHASE problem over the source map"""
    cin, cout = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3)
    out = _f16(4, cout, 4 * cin, device=w.device)
    if ovf is not None:
        L.check(L.lib().ctrl_op_pack_convt_w_phase_ovf(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cin, cout, L.ptr(ovf), L.cur_stream()))
        return out
    L.check(L.lib().ctrl_op_pack_convt_w_phase(L.ptr(w.contiguous()), L.dtype_code(w.dtype), L.ptr(out), cin, cout, L.cur_stream()))
    return out


def lineart_launch_shape(kernel, Cc=0):
    a, b = C.c_int(), C.c_int()
    L.check(L.lib().ctrl_lineart_launch_shape(int(kernel), int(Cc), C.byref(a), C.byref(b)))
    return a.value, b.value


def lineart_stem_into(src_u8, w_packed, out, flag=None):
    """src uint8 [N][H][W][3], w fp32 [49][3][64] -> out fp16 [N][H][W][64]"""
    N, H, W = src_u8.shape[:3]
    L.check(L.lib().ctrl_op_lineart_stem(L.ptr(src_u8), N, H, W, L.ptr(w_packed), L.ptr(out), L.ptr(flag), L.cur_stream()))


def in_stats_ws_floats(N, HW, Cc):
    """floats of scratch in_stats_into needs (0: a shape it refuses)"""
    return int(L.lib().ctrl_op_in_stats_ws_floats(int(N), int(HW), int(Cc)))


def in_stats_into(x, N, HW, Cc, stats, ws=None):
    """x fp16 [N][HW][C] -> stats fp32 [N][C][2] = (sum, sum of squares)"""
    if ws is None:
        ws = torch.empty(in_stats_ws_floats(N, HW, Cc) + 4, dtype=torch.float32, device=x.device)
    L.check(L.lib().ctrl_op_in_stats(L.ptr(x), N, HW, Cc, L.ptr(stats), L.ptr(ws), L.cur_stream()))


def in_apply_into(x, stats, N, H, W, Cc, out, pad=0, relu=False, res=None, res_pad=0, eps=1e-5, flag=None):
    """InstanceNorm apply: out fp16 [N][H + 2 pad][W + 2 pad][C] (reflection padding written out)"""
    L.check(L.lib().ctrl_op_in_apply(L.ptr(x), L.ptr(stats), N, H, W, Cc, float(eps), int(bool(relu)), L.ptr(res), int(res_pad), int(pad),
                                     L.ptr(out), L.ptr(flag), L.cur_stream()))


def lineart_head_into(xp, N, H, W, w_packed, bias, out, logits=None):
    """xp fp16 [N][H + 6][W + 6][64], w fp32 [49][64] -> out uint8 [N][H][W] | [N][H][W][3] (+ fp32 logits)"""
    ch = 3 if out.dim() == 4 else 1
    L.check(L.lib().ctrl_op_lineart_head(L.ptr(xp), N, H, W, L.ptr(w_packed), float(bias), ch, L.ptr(out), L.ptr(logits), L.cur_stream()))


_profiling = False


def profiling():
    """True while a Profiler block records (one kernel at a time: the mirrors keep to one stream then)"""
    return _profiling


class Profiler:
    """HIP-event profiler over kernel classes (see ctrl_prof_* in include/ctrl_hip.h)."""

    def __enter__(self):
        global _profiling
        L.check(L.lib().ctrl_prof_begin())
        _profiling = True
        return self

    def __exit__(self, *exc):
        global _profiling
        _profiling = False
        lib = L.lib()
        L.check(lib.ctrl_prof_end())
        self.rows = {}
        name = C.create_string_buffer(64)
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int()
        for i in range(lib.ctrl_prof_count()):
            L.check(lib.ctrl_prof_get(i, name, 64, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            self.rows[name.value.decode()] = (ms.value, n.value, fl.value, by.value)
        # per-launch records, in launch order: (class tag, kernel symbol, shape note, ms, flops, bytes, grid work-items)
        self.launches = []
        tag, sym, det = C.create_string_buffer(64), C.create_string_buffer(256), C.create_string_buffer(256)
        grid = C.c_int64()
        for i in range(lib.ctrl_prof_launch_count()):
            L.check(lib.ctrl_prof_launch_get(i, tag, 64, sym, 256, det, 256, C.byref(ms), C.byref(fl), C.byref(by), C.byref(grid)))
            self.launches.append((tag.value.decode(), sym.value.decode(), det.value.decode(), ms.value, fl.value, by.value, grid.value))
        return False

    def per_kernel(self, reps=1):
        """launches grouped by (kernel symbol, shape): {key: dict(tag, symbol, shape, launches_per_step, ms_per_step,
        avg_launch_ms, flops_per_launch, bytes_per_launch, tflops, gbs, grid)} -- one row per template instantiation x shape"""
        acc = {}
        for tag, sym, det, ms, fl, by, grid in self.launches:
            k = (sym, det)
            a = acc.setdefault(k, dict(tag=tag, symbol=sym, shape=det, n=0, ms=0.0, flops=0.0, bytes=0.0, grid=grid))
            a["n"] += 1; a["ms"] += ms; a["flops"] += fl; a["bytes"] += by
        out = {}
        for (sym, det), a in acc.items():
            n, ms = a["n"], a["ms"]
            out[(sym + " " + det).strip()] = dict(
                tag=a["tag"], symbol=sym, shape=det, launches_per_step=n / reps, ms_per_step=ms / reps, avg_launch_ms=ms / n,
                flops_per_launch=a["flops"] / n, bytes_per_launch=a["bytes"] / n, grid=a["grid"],
                tflops=(a["flops"] / (ms * 1e-3) / 1e12) if a["flops"] and ms > 0 else None,
                gbs=(a["bytes"] / (ms * 1e-3) / 1e9) if a["bytes"] and ms > 0 else None)
        return out
