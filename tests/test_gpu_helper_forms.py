"""The layout, packing and small helper kernels (csrc/elementwise.hip; unet_conv_out, i2v_frames of csrc/unet.hip; vae_conv_in,
vae_row_softmax of csrc/vae.hip) on the GPU: every case of tests/helper_forms.py through the C entry points, against the exact
restatements bit for bit or against the fp64 references and their element-wise bounds.  Every output lies inside a poisoned allocation
(helpers.Guarded), so a strided, partial or scattered result also proves that nothing outside it was written; inputs are surrounded by
NaN.  The checks themselves are tested on the host (tests/test_helper_check_host.py).  Nothing here provokes a fault: every refused call
returns before a launch.  One PARITY line per kernel gives the worst share of its bound."""
import ctypes as C

import pytest
import torch

import helpers
import helper_forms as H
from helpers import Guarded

pytestmark = pytest.mark.gpu
F32, F16, BF16, I32 = torch.float32, torch.float16, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def L_(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def ops(L_):
    from ctrl_adapter_amd import ops
    return ops


def _inp(t, dev, pad_cols=0):
    """an input inside NaN: one slab (1-D: 8 elements) before and after along the first axis, `pad_cols` NaN columns after the last"""
    if t.dim() == 1:
        return Guarded.inp(t, (8,), (8,), dev)
    before = (1,) + (0,) * (t.dim() - 1)
    return Guarded.inp(t, before, (1,) + (0,) * (t.dim() - 2) + (pad_cols,), dev)


def _out(shape, dt, dev, pad_cols=0):
    """an output inside poison: one slab (1-D: 8 elements) before and after along the first axis, `pad_cols` poison columns"""
    shape = tuple(shape)
    if len(shape) == 1:
        return Guarded.out((shape[0] + 16,), (slice(8, 8 + shape[0]),), dt, dev)
    full = (shape[0] + 2,) + shape[1:-1] + (shape[-1] + pad_cols,)
    valid = (slice(1, 1 + shape[0]),) + tuple(slice(0, s) for s in shape[1:])
    return Guarded.out(full, valid, dt, dev)


def _untouched(what, *gs):
    torch.cuda.synchronize()
    for g in gs:
        if g is not None:
            g.assert_untouched(what)


def _exact(what, got, want, nan_is_nan=False):
    """bit for bit; nan_is_nan: a NaN must come back as a NaN in the same place, whatever its sign and payload (the other elements bit
    for bit)"""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if nan_is_nan:
        gn, wn = torch.isnan(got), torch.isnan(want)
        assert bool(wn.any()) and torch.equal(gn, wn), "%s: NaNs at %s, wanted at %s" % (what, gn.nonzero().tolist(), wn.nonzero().tolist())
        print("NaN through %s: bits %s (restated: %s)" % (what, [hex(int(v) & 0xFFFF) for v in helpers._bits(got[gn])],
                                                          [hex(int(v) & 0xFFFF) for v in helpers._bits(want[wn])]))
        got, want = torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want)
    diff = helpers._bits(got.contiguous()) != helpers._bits(want.contiguous())
    if bool(diff.any()):
        first = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ from the exact restatement; first at %s: got %r want %r" % (
            what, int(diff.sum()), diff.numel(), first, float(got[first]), float(want[first])))


class Worst:
    """collects the worst |err| / bound of a kernel's cases and every failure; one PARITY line at the end"""

    def __init__(self, kernel):
        self.kernel, self.worst, self.n, self.fails = kernel, 0.0, 0, []

    def close(self, what, out, ref, bound):
        o = out.detach().cpu().double()
        assert o.shape == ref.shape, (what, tuple(o.shape), tuple(ref.shape))
        self.n += 1
        if not bool(torch.isfinite(o).all()):
            self.fails.append("%s: %d non-finite outputs" % (what, int((~torch.isfinite(o)).sum())))
            return
        err = (o - ref).abs()
        w = float((err / bound).max())
        self.worst = max(self.worst, w)
        bad = err > bound
        if bool(bad.any()):
            first = tuple(int(v) for v in bad.nonzero()[0])
            self.fails.append("%s: %d of %d elements beyond the bound (worst err/bound %.2f); first at %s: got %.8g want %.8g bound %.3g" % (
                what, int(bad.sum()), bad.numel(), w, first, float(o[first]), float(ref[first]), float(bound[first])))

    def exact(self, what, got, want, nan_is_nan=False):
        self.n += 1
        try:
            _exact(what, got, want, nan_is_nan)
        except AssertionError as e:
            self.fails.append(str(e))

    def done(self, exact_only=False):
        print("PARITY %-22s %4d cases  %s" % (self.kernel, self.n, "bit-exact" if exact_only else "worst err/bound %.3f" % self.worst))
        assert not self.fails, "%s: %d failing cases:\n%s" % (self.kernel, len(self.fails), "\n".join(self.fails[:12]))


# ---------------------------------------------------------------------------------------------------------------------------
# transposes
# ---------------------------------------------------------------------------------------------------------------------------
def test_nchw_to_nhwc(L_, gpu):
    w = Worst("nchw_to_nhwc")
    for c in H.TRANSPOSE:
        if c.map is not None or c.special:
            continue
        x, want = H.to_nhwc_problem(c)
        gx, gy = _inp(x, gpu), _out((c.N, c.HW, c.C), F16, gpu)
        L_.check(L_.lib().ctrl_op_nchw_to_nhwc(L_.ptr(gx.view), L_.dtype_code(c.dt), L_.ptr(gy.view), c.N, c.C, c.HW, L_.cur_stream()))
        w.exact(c.id, gy.view, want)
        _untouched(c.id, gx, gy)
    w.done(True)


def test_nhwc_to_nchw_with_scale_and_image_map(L_, ops, gpu):
    """one product and one conversion: bit for bit, in every output type and scale; with an image map the images nothing maps to keep
    their poison.  The bf16 store rounds a NaN as a number (f32_to_bf16, csrc/common.h): the canonical NaN and +-inf survive it, which
    is what `tr-special-bf16` holds; a NaN whose upper seven mantissa bits are all ones and whose lower sixteen round up would carry into
    +-0 -- no kernel produces one.  A NaN's sign and payload are not part of the restatement (the host's own conversions differ in them)."""
    w = Worst("nhwc_to_nchw")
    for c in H.TRANSPOSE:
        x, want = H.to_nchw_problem(c)
        gx, gy = _inp(x, gpu), _out((c.ndst, c.C, c.HW), c.dt, gpu)
        m = torch.tensor(c.map, dtype=I32, device=gpu) if c.map else None
        ops.nhwc_to_nchw_into(gx.view, gy.view, c.N, c.C, c.HW, c.scale, m)
        w.exact(c.id, gy.view, want, nan_is_nan=bool(c.special))
        _untouched(c.id, gx, gy)
        if c.special:
            got = gy.view.cpu().float().reshape(-1)
            assert bool(torch.isnan(got[0])) and float(got[c.HW]) == float("inf") and float(got[2 * c.HW]) == float("-inf")
    # no map through the old entry point: the same bits
    c = H.pick(H.TRANSPOSE, C=70, HW=130, N=3)
    x, want = H.to_nchw_problem(c)
    y = ops.nhwc_to_nchw(x.to(gpu).reshape(c.N, c.HW, 1, c.C), dtype=c.dt, scale=c.scale)
    w.exact(c.id + " (ctrl_op_nhwc_to_nchw)", y.reshape(c.N, c.C, c.HW), want)
    w.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# avgpool, sincos
# ---------------------------------------------------------------------------------------------------------------------------
def _avgpool(L_, dev, x, shape, NC, dt):
    Hin, Win, Hout, Wout = shape
    gx, gy = _inp(x, dev), _out((NC, Hout, Wout), dt, dev)
    L_.check(L_.lib().ctrl_avgpool_nchw(L_.ptr(gx.view), L_.ptr(gy.view), L_.dtype_code(dt), NC, Hin, Win, Hout, Wout, L_.cur_stream()))
    return gx, gy


def test_avgpool(L_, gpu):
    w = Worst("avgpool")
    for c in H.AVGPOOL:
        x, ref, bound = H.avgpool_problem(c)
        gx, gy = _avgpool(L_, gpu, x, c.shape, c.NC, c.dt)
        w.close(c.id, gy.view, ref, bound)
        _untouched(c.id, gx, gy)
    w.done()


def test_avgpool_second_grid_stride_trip(L_, gpu):
    x, want = H.avgpool_second_trip()
    gx, gy = _avgpool(L_, gpu, x, H.AP_SECOND.shape, 1, F16)
    _exact(H.AP_SECOND.id, gy.view, want)
    _untouched(H.AP_SECOND.id, gy)
    print("PARITY %-22s second trip (%d outputs) bit-exact" % ("avgpool", want.numel()))


def test_timestep_sincos(L_, gpu):
    w = Worst("sincos")
    for c in H.SINCOS:
        for which in range(4):
            t, ref, bound, _ = H.sincos_problem(c, which)
            gt, gy = _inp(t, gpu), _out((c.N, c.dim), F32, gpu)
            L_.check(L_.lib().ctrl_op_timestep_sincos(L_.ptr(gt.view), c.t_count, L_.ptr(gy.view), c.N, c.dim, L_.cur_stream()))
            w.close("%s t%d" % (c.id, which), gy.view, ref, bound)
            _untouched(c.id, gt, gy)
    w.done()


# ---------------------------------------------------------------------------------------------------------------------------
# linear_small and its grouped form
# ---------------------------------------------------------------------------------------------------------------------------
def test_linear_small_and_group(L_, ops, gpu):
    """x rows K + 4 apart, out rows N + 3 apart; the grouped kernel gives the same bits"""
    w = Worst("linear_small")
    dev_ops = {}
    for c in H.LINEAR:
        if (c.N, c.K) not in dev_ops:
            x, W, b = H.linear_operands(c.N, c.K)
            dev_ops[(c.N, c.K)] = (_inp(x, gpu, 4), _inp(W, gpu), _inp(b, gpu))
        gx, gW, gb = dev_ops[(c.N, c.K)]
        ref, bound = H.linear_reference(c)
        outs = []
        for grouped in (False, True):
            gy = _out((c.M, c.N), F32, gpu, 3)
            args = (gx.view, c.K + 4, gW.view, gb.view if c.bias else None, gy.view, c.N + 3, c.M, c.N, c.K, c.in_silu, c.out_silu)
            if grouped:
                ops.linear_small_group([ops.small_lin(*args)])
            else:
                ops.linear_small_into(*args)
            _untouched(c.id, gy)
            outs.append(gy.view.cpu())
        w.close(c.id, outs[0], ref, bound)
        w.exact(c.id + " (group)", outs[1], outs[0])
    _untouched("linear_small inputs", *[g for t in dev_ops.values() for g in t])
    w.done()


# ---------------------------------------------------------------------------------------------------------------------------
# blend, add_rowvec
# ---------------------------------------------------------------------------------------------------------------------------
def test_blend(L_, ops, gpu):
    w = Worst("blend")
    for c in H.BLEND:
        a, b, ref, bound = H.blend_problem(c)
        ga, gb, gm, gy = _inp(a, gpu), _inp(b, gpu), _inp(torch.tensor([c.mix], dtype=F32), gpu), _out((a.numel(),), c.y, gpu)
        ops.blend_into(ga.view, gb.view, gm.view, gy.view)
        w.close(c.id, gy.view, ref, bound)
        _untouched(c.id, ga, gb, gm, gy)
    w.done()


def test_blend_second_grid_stride_trip(L_, ops, gpu):
    a, b, want = H.blend_second_trip()
    gy = _out((a.numel(),), F16, gpu)
    ops.blend_into(a.to(gpu), b.to(gpu), torch.zeros(1, device=gpu), gy.view)
    _exact("blend second trip", gy.view, want)
    _untouched("blend second trip", gy)
    print("PARITY %-22s second trip (%d chunks) bit-exact" % ("blend", H.BL_SECOND_CHUNKS))


def _add_rowvec(ops, dev, c):
    x, v, want = H.addv_problem(c)
    gv = _inp(v, dev, 4)
    if c.inplace:
        gy = _out((c.M, c.C), c.y, dev)
        gy.view.copy_(x)
        gx = gy
    else:
        gx, gy = _inp(x, dev), _out((c.M, c.C), c.y, dev)
    ops.add_rowvec_into(gx.view, gv.view, c.C + 4, gy.view, c.M, c.C, c.rows_per_img, c.vmod)
    _exact(c.id, gy.view, want)
    _untouched(c.id, gv, gy, None if c.inplace else gx)


def test_add_rowvec(L_, ops, gpu):
    """one fp32 add and one conversion: bit for bit; v rows C + 4 apart, one row more than vmod behind them"""
    for c in H.ADDV:
        _add_rowvec(ops, gpu, c)
    _add_rowvec(ops, gpu, H.AV_SECOND)
    print("PARITY %-22s %4d cases  bit-exact (one of them %d chunks: the second trip)" % ("add_rowvec", len(H.ADDV) + 1, H.AV_SECOND.M))


# ---------------------------------------------------------------------------------------------------------------------------
# merge, router
# ---------------------------------------------------------------------------------------------------------------------------
def _merge(L_, dev, xs, wdev, widx, dt, n):
    K = len(xs)
    gy = _out((n,), dt, dev)
    ptrs = (C.c_void_p * K)(*[x.data_ptr() for x in xs])
    idx = (C.c_int * K)(*widx)
    L_.check(L_.lib().ctrl_router_merge(ptrs, L_.ptr(wdev), idx, K, L_.ptr(gy.view), L_.dtype_code(dt), C.c_size_t(n), L_.cur_stream()))
    return gy


def test_router_merge_and_merge_gather_agree(L_, ops, gpu):
    """merge_kernel against fp64, and bit for bit the one-slot identity-map merge_gather on the same inputs.  `mg-special-bf16`: weight 1
    over the canonical NaN, +-inf and 3e38 through the bf16 cast (f32_to_bf16 rounds a NaN as a number; these survive)."""
    w = Worst("merge")
    for c in H.MERGE:
        xs, wt, widx, ref, bound = H.merge_problem(c)
        gxs, gw = [_inp(x, gpu) for x in xs], _inp(wt, gpu)
        gy = _merge(L_, gpu, [g.view for g in gxs], gw.view, widx, c.dt, c.n)
        if c.special:
            w.exact(c.id, gy.view, xs[0], nan_is_nan=True)
        else:
            w.close(c.id, gy.view, ref, bound)
        _untouched(c.id, gw, gy, *gxs)
        other = ops.merge_gather([[g.view.reshape(1, c.n) for g in gxs]], weights=gw.view.reshape(1, c.E).contiguous(), rows=[0], widx=widx)[0]
        w.exact(c.id + " (merge_gather)", other.reshape(-1), gy.view.cpu(), nan_is_nan=bool(c.special))
    w.done()


def test_router_merge_second_grid_stride_trip(L_, gpu):
    n = H.MG_SECOND_N
    x = H.odd_values((n,), F16, H._gen("mg2"))
    gy = _merge(L_, gpu, [x.to(gpu)], torch.tensor([0.0, 1.0], device=gpu), [1], F16, n)
    _exact("merge second trip", gy.view, x)
    _untouched("merge second trip", gy)
    print("PARITY %-22s second trip (%d elements) bit-exact" % ("merge", n))


def test_router_softmax(L_, gpu):
    w = Worst("router_softmax")
    for c in H.ROUTER:
        wg, m, ref, bound, dead = H.router_problem(c)
        gw = _inp(wg, gpu) if wg is not None else None
        gy = _out((c.R, c.E), F32, gpu)
        mask = (C.c_int * c.E)(*m) if m is not None else None
        L_.check(L_.lib().ctrl_router_weights(L_.ptr(gw.view) if gw else None, mask, L_.ptr(gy.view), c.R, c.E, int(c.equal), L_.cur_stream()))
        out = gy.view.cpu()
        w.close(c.id, out, ref, bound)
        assert bool((out[:, dead] == 0).all()), "%s: a masked expert beside a live one must be exactly 0" % c.id
        _untouched(c.id, gw, gy)
    w.done()


# ---------------------------------------------------------------------------------------------------------------------------
# packers and the fp16 range guard
# ---------------------------------------------------------------------------------------------------------------------------
def _pack(L_, dev, sym, src, out_shape, out_dt, dims, ovf=None):
    gs, go = _inp(src.reshape(-1), dev), _out((int(torch.tensor(out_shape).prod()),), out_dt, dev)
    args = [L_.ptr(gs.view), L_.dtype_code(src.dtype), L_.ptr(go.view)] + list(dims)
    if ovf is not None:
        sym, args = sym + "_ovf", args + [L_.ptr(ovf)]
    L_.check(getattr(L_.lib(), sym)(*args, L_.cur_stream()))
    torch.cuda.synchronize()
    gs.assert_untouched(sym)
    go.assert_untouched(sym)
    return go.view.cpu().reshape(out_shape)


def test_weight_packers(L_, gpu):
    w = Worst("pack_*")
    for c in H.PK_CONV:
        src = H.pack_source(c, H.conv_w_shape(c))
        dims = (c.Cout, c.Cin, c.taps)
        w.exact(c.id, _pack(L_, gpu, "ctrl_op_pack_conv_w", src, (c.Cout, c.taps, c.Cin), F16, dims), H.pack_conv_expect(src))
        w.exact(c.id + " dup", _pack(L_, gpu, "ctrl_op_pack_conv_w_dup", src, (c.Cout, c.taps, 2 * c.Cin), F16, dims), H.pack_conv_dup_expect(src))
        if c.taps == 9:
            w.exact(c.id + " phase", _pack(L_, gpu, "ctrl_op_pack_conv_w_phase", src, (4, c.Cout, 4, c.Cin), F16, dims[:2]), H.pack_phase_expect(src))
    for c in H.PK_DIRECT:
        src = H.pack_source(c, (c.Cout, c.Cin, 3, 3))
        w.exact(c.id, _pack(L_, gpu, "ctrl_op_pack_conv_w_direct", src, (9, c.Cin, c.Cout), F32, (c.Cout, c.Cin)), H.pack_direct_expect(src))
    for c in H.PK_LINEAR + [H.PK_LINEAR_SECOND]:
        src = H.pack_source(c, (c.N, c.K))
        w.exact(c.id, _pack(L_, gpu, "ctrl_op_pack_linear_w", src, (c.N, c.K), F16, (c.N, c.K, int(c.geglu))), H.pack_linear_expect(src, c.geglu))
    for c in H.PK_VEC:
        src = H.pack_source(c, (c.N,))
        w.exact(c.id, _pack(L_, gpu, "ctrl_op_pack_vec", src, (c.N,), F32, (c.N, int(c.geglu))), H.pack_vec_expect(src, c.geglu))
    w.done(True)


_OVF = {"conv": ("ctrl_op_pack_conv_w", lambda r, c, t: (r, c, t), lambda r, c, t: r * c * t),
        "dup": ("ctrl_op_pack_conv_w_dup", lambda r, c, t: (r, c, t), lambda r, c, t: 2 * r * c * t),
        "phase": ("ctrl_op_pack_conv_w_phase", lambda r, c, t: (r, c), lambda r, c, t: 16 * r * c),
        "linear": ("ctrl_op_pack_linear_w", lambda r, c, t: (r, c, 0), lambda r, c, t: r * c)}


def _flag_after(L_, dev, kind, src, shape):
    sym, dims, n_out = _OVF[kind]
    flag = Guarded.out((3,), (slice(1, 2),), I32, dev)
    flag.view.zero_()
    _pack(L_, dev, sym, src, (n_out(*shape),), F16, dims(*shape), ovf=flag.view)
    flag.assert_untouched(kind)
    return int(flag.view.cpu()[0])


def test_fp16_range_flag_of_the_packers(L_, gpu):
    """The guard judges the fp32 value BEFORE the rounding: 65519 rounds to 65504 in fp16 and is flagged all the same; +-65504 is not.
    From fp32 and bf16 sources, the offending element first, last, and (on shapes of more than 8192 * 256 outputs) beyond the first
    grid-stride trip; the phase pack is judged on its sums."""
    n = 0
    for kind in H.OVF_KINDS:
        for dt, rows in H.OVF_VALUES.items():
            for value, want in rows:
                for where in ("first", "last"):
                    src = H.ovf_source(kind, H.OVF_SMALL[kind], dt, value, where)
                    assert H.ovf_expected(kind, src) == want
                    assert _flag_after(L_, gpu, kind, src, H.OVF_SMALL[kind]) == want, (kind, dt, value, where)
                    n += 1
        for dt, value in ((F32, None), (F32, 65505.0), (BF16, 65536.0)):
            src = H.ovf_source(kind, H.OVF_SECOND[kind], dt, value, "second")
            assert _flag_after(L_, gpu, kind, src, H.OVF_SECOND[kind]) == int(value is not None), (kind, dt, value, "second trip")
            n += 1
    for dt in (F32, BF16):          # every tap fits, a phase sum does not
        src = H.ovf_phase_sum_source(dt)
        assert [_flag_after(L_, gpu, k, src, (2, 3, 9)) for k in ("conv", "dup", "phase")] == [0, 0, 1], dt
    # a flag that is already set stays set
    sym, dims, n_out = _OVF["linear"]
    flag = torch.ones(1, dtype=I32, device=gpu)
    _pack(L_, gpu, sym, H.ovf_source("linear", (5, 40, 1), F32, None, "first"), (200,), F16, (5, 40, 0), ovf=flag)
    assert int(flag.cpu()[0]) == 1
    print("PARITY %-22s %4d cases  flag as restated" % ("fp16 range guard", n + 7))


def test_a_plan_refuses_a_weight_outside_the_fp16_range(L_, gpu):
    """the smallest plan of the suite (the tiny KL-VAE encoder) with one fp32 weight at 7e4 is refused at creation with the packers'
    message; at 65504 it loads"""
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    from vae_encoder_ref import TINY
    sd = {k: v.clone() for k, v in seeded_init(P.AutoencoderKLEncoder(**TINY), seed=3).state_dict().items()}
    for value, ok in ((7.0e4, False), (65504.0, True)):
        sd[H.PLAN_WEIGHT].view(-1)[-1] = value
        m = P.AutoencoderKLEncoder(**TINY)
        m.load_state_dict(sd)
        m = m.to(gpu)
        if ok:
            with torch.cuda.device(gpu):
                assert m._ensure_plan()
        else:
            with pytest.raises(RuntimeError, match="outside the fp16 range"), torch.cuda.device(gpu):
                m._ensure_plan()


# ---------------------------------------------------------------------------------------------------------------------------
# the per-pixel kernels only a plan reached
# ---------------------------------------------------------------------------------------------------------------------------
def test_unet_conv_out(L_, ops, gpu):
    w = Worst("unet_conv_out")
    for c in H.CONV_OUT:
        x, wt, b, ref, bound = H.conv_out_problem(c.id)
        gx, gb = _inp(x, gpu), _inp(b, gpu)
        wd = ops.pack_conv_w_direct(wt.to(gpu))
        gy = _out((ref.numel(),), c.dt, gpu)
        ops.unet_conv_out(gx.view, wd, gb.view, gy.view, c.N, c.H, c.W, c.C, c.Cout, c.layout, c.F)
        w.close(c.id, gy.view.reshape(ref.shape), ref, bound)
        _untouched(c.id, gx, gb, gy)
    w.done()


def test_i2v_frames(L_, ops, gpu):
    w = Worst("i2v_frames")
    for c in H.I2V:
        x, want = H.i2v_problem(c)
        gx, gy = _inp(x, gpu), _out((c.B * c.F, 4, c.HW), F32, gpu)
        ops.i2v_frames(gx.view, gy.view, c.B, c.F, c.HW)
        w.exact(c.id, gy.view, want)
        _untouched(c.id, gx, gy)
    # the form the plan uses for the embedding: B = F = 1 over HW = n / 4 elements is a plain conversion
    x = H.odd_values((1, 4, 1, 77), BF16, H._gen("i2v-emb"))
    gy = _out((1, 4, 77), F32, gpu)
    ops.i2v_frames(x.to(gpu), gy.view, 1, 1, 77)
    w.exact("i2v-embedding-form", gy.view, x.float().reshape(1, 4, 77))
    w.done(True)


def test_vae_conv_in(L_, ops, gpu):
    w = Worst("vae_conv_in")
    for c in H.CONV_IN:
        px, wt, b, ref, bound = H.conv_in_problem(c.id)
        gp, gb = _inp(px, gpu), _inp(b, gpu)
        wd = ops.pack_conv_w_direct(wt.to(gpu))
        gy = _out((c.H * c.W * c.Cout,), F32, gpu)
        ops.vae_conv_in(gp.view, wd, gb.view, gy.view, c.H, c.W, c.Cout)
        w.close(c.id, gy.view.reshape(ref.shape), ref, bound)
        _untouched(c.id, gp, gb, gy)
    w.done()


def test_vae_row_softmax(L_, ops, gpu):
    """score rows L + 4 apart, P rows Lpad + 8 apart; the pad columns are +0 bit for bit; a constant row is fp16(1 / L) and a row with one
    entry 80 above the rest is 1 beside exact zeros"""
    w = Worst("vae_row_softmax")
    for c in H.SOFTMAX:
        S, ref, bound, exact = H.softmax_problem(c.id)
        gs, gp = _inp(S, gpu, 4), _out((c.rows, c.Lpad), F16, gpu, 8)
        ops.vae_row_softmax(gs.view, c.L + 4, gp.view, c.Lpad + 8, c.rows, c.L, c.Lpad)
        out = gp.view.cpu()
        w.close(c.id, out[:, :c.L], ref, bound)
        if exact is not None:
            w.exact(c.id + " (exact)", out[:, :c.L].contiguous(), exact)
        assert bool((helpers._bits(out[:, c.L:].contiguous()) == 0).all()), "%s: the pad columns must be +0" % c.id
        _untouched(c.id, gs, gp)
    w.done()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(L_, gpu):
    """every refused call names the same poisoned buffer for all of its tensors: it comes back untouched"""
    g = Guarded.out((4096,), (slice(1024, 3072),), F32, gpu)
    ptr = g.view.data_ptr()
    assert ptr % 16 == 0
    for name, sym, args, msg in H.refusals(ptr, ptr + 2):
        rc = getattr(L_.lib(), sym)(*args, L_.cur_stream())
        err = (L_.lib().ctrl_last_error() or b"").decode()
        assert rc != 0 and msg in err, (name, rc, err)
    torch.cuda.synchronize()
    snap = g._snap
    assert torch.equal(helpers._bits(g.buf), snap), "a refused call wrote"
