"""The lineart annotator on the GPU (csrc/lineart.hip, csrc/plan_lineart.cpp, ctrl_adapter_amd.lineart) against tests/lineart_ref.py.

Kernel forms, each inside poisoned surroundings and against its fp64 reference with the element-wise bound of lineart_ref (nothing is
measured, there is no slack factor): the stem and the head at the tile edges ctrl_lineart_launch_shape reports, the InstanceNorm statistics
and apply kernels at their chunk edges in all three output layouts, the transposed convolution as the implicit GEMM's phase form and the
valid 3x3 form (tap_origin = 1, stride 1, Hin = Hout + 2) in both kernel families with helpers.igemm_bound.  The plan is bit-identical to
its kernels chained by hand, so nothing between the kernels goes unchecked.  The whole detector on the calibrated checkpoint: every logit
within 4 x max |emulated - fp64| of the fp64 restatement (the tolerance tests/test_lineart_host.py proves the planted errors against).
Figures are printed before they are asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import lineart_forms as LF
import lineart_ref as R
from helpers import Guarded

pytestmark = pytest.mark.gpu
U8, F16, F32 = torch.uint8, torch.float16, torch.float32
U8_POISON = 0xA5


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


@pytest.fixture(scope="module")
def tiles(ops):
    return [ops.lineart_launch_shape(0), ops.lineart_launch_shape(1)]


def _guard(shape, dtype, dev, data=None, before=128, after=192):
    """a contiguous tensor of `shape` inside a flat allocation (16-byte aligned start); an output's surroundings hold a fixed pattern that
    must come back, an input's hold NaN (uint8: 255) and must not be written either"""
    n = int(np.prod(shape))
    if data is None:
        fill = U8_POISON if dtype == U8 else helpers._POISON[dtype]
    else:
        fill = 255 if dtype == U8 else float("nan")
    g = Guarded((before + n + after,), (slice(before, before + n),), dtype, dev, fill)
    if data is not None:
        g.view.copy_(torch.as_tensor(data).reshape(-1).to(dtype))
        g.is_input = True
    g._snap = helpers._bits(g.buf).clone()
    g.t = g.view.view(*shape)
    return g


def _check(got, ref, bound, what):
    """every element of got (fp64 CPU) finite and within bound of ref; returns the worst |err| / bound"""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite outputs" % (what, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print("LINEART-CHECK %-58s worst err/bound %.3f  rel_inf %.2e" % (what, worst, float(err.max() / ref.abs().max().clamp_min(1e-12))))
    bad = err > bound
    assert not bool(bad.any()), "%s: %d of %d elements beyond the bound (worst %.2f); first at %s" % (
        what, int(bad.sum()), bad.numel(), worst, tuple(int(v) for v in bad.nonzero()[0]))
    return worst


def _nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).double().cpu()


# ---------------------------------------------------------------------------------------------------------------- stem
def _run_stem(ops, gpu, fr, w):
    N, H, W = fr.shape[:3]
    src = _guard((N, H, W, 3), U8, gpu, fr)
    wp = _guard((147 * 64,), F32, gpu, R.pack_stem(w))
    out = _guard((N, H, W, 64), F16, gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    ops.lineart_stem_into(src.t, wp.t, out.t, flag)
    torch.cuda.synchronize()
    for gd in (src, wp, out):
        gd.assert_untouched("stem %dx%dx%d" % (N, H, W))
    assert int(flag[0]) == 0
    return out.t


def test_stem_channel_order_and_padding(ops, gpu):
    """a frame whose three channels differ: only RGB / 255 under REFLECTION padding stays inside the bound"""
    fr, w = LF.stem_problem(2, 24, 40)
    fr[0, :8, :8] = torch.tensor([255, 0, 0], dtype=U8)          # three plain colours meet at the corner the reflection folds
    fr[0, :8, 8:16] = torch.tensor([0, 255, 0], dtype=U8)
    fr[0, 8:16, :8] = torch.tensor([0, 0, 255], dtype=U8)
    got = _nchw(_run_stem(ops, gpu, fr, w))
    ref, bound = R.stem_ref(fr, w)
    _check(got, ref, bound, "stem three colours")
    swapped, _ = R.stem_ref(fr, w, bgr=True)
    assert int(((swapped - ref).abs() > bound).sum()) > ref.numel() // 2          # the check tells the orders apart
    zero, _ = R.stem_ref(fr, w, zero_pad=True)
    assert int(((zero - ref).abs() > bound).sum()) > 2 * (24 + 40) * 64


def test_stem_forms(ops, gpu, tiles):
    worst = 0.0
    sizes = LF.tile_sizes(*tiles[0])
    for N in LF.BATCHES:
        for H, W in sizes:
            fr, w = LF.stem_problem(N, H, W)
            ref, bound = R.stem_ref(fr, w)
            worst = max(worst, _check(_nchw(_run_stem(ops, gpu, fr, w)), ref, bound, "stem %dx%dx%d" % (N, H, W)))
    print("PARITY lineart stem: worst |err| / bound %.3f over %d sizes x %s frames" % (worst, len(sizes), LF.BATCHES))


def test_stem_raises_the_range_flag(ops, gpu):
    fr, w = LF.stem_problem(1, 8, 16)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    out = torch.empty((1, 8, 16, 64), dtype=F16, device=gpu)
    ops.lineart_stem_into(fr.to(gpu), R.pack_stem(w * 2.0 ** 20).to(gpu), out, flag)
    torch.cuda.synchronize()
    assert int(flag[0]) == 1


# ---------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("ch", [1, 3])
def test_head_forms(ops, gpu, tiles, ch):
    """logits inside the fp64 bound; every byte the byte of some logit inside it (no element is left out)"""
    worst = 0.0
    for N in LF.BATCHES:
        for H, W in LF.tile_sizes(*tiles[1]):
            x, w, b = LF.head_problem(N, H, W)
            xp = R.reflect_pad(x.float(), 3).half()
            xg = _guard((N, H + 6, W + 6, 64), F16, gpu, R.nhwc(xp))
            wg = _guard((49 * 64,), F32, gpu, R.pack_head(w))
            out = _guard((N, H, W) if ch == 1 else (N, H, W, 3), U8, gpu, before=96, after=96)
            lg = _guard((N, H, W), F32, gpu)
            ops.lineart_head_into(xg.t, N, H, W, wg.t, float(b[0]), out.t, lg.t)
            torch.cuda.synchronize()
            what = "head ch%d %dx%dx%d" % (ch, N, H, W)
            ref, bound = R.head_ref(xp, w, b)
            worst = max(worst, _check(lg.t.double().cpu(), ref, bound, what))
            got = out.t.cpu().numpy()
            first = got if ch == 1 else got[..., 0]
            bad = R.u8_failures(first, ref.numpy(), bound.numpy())
            lo, hi = R.u8_interval(ref.numpy(), bound.numpy())
            single = float((hi == lo).mean())
            print("LINEART-HEAD %s: logit std %.2f, %d levels, %d bytes outside; widest interval %d, %.1f %% of the pixels admit one byte only" % (
                what, float(ref.std()), len(np.unique(first)), bad, int((hi - lo).max()), 100 * single))
            assert bad == 0
            if H * W >= 128:
                assert len(np.unique(first)) > 20
            if ch == 3:
                assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
            for gd in (xg, wg, out, lg):
                gd.assert_untouched(what)
    print("PARITY lineart head<%d>: worst logit |err| / bound %.3f" % (ch, worst))


# ---------------------------------------------------------------------------------------------------------------- InstanceNorm
@pytest.mark.parametrize("Cw", LF.IN_WIDTHS)
def test_instance_norm_forms(ops, gpu, Cw):
    rpb, _ = ops.lineart_launch_shape(2, Cw)
    worst_s = worst_a = 0.0
    for H, W in LF.in_sizes(rpb):
        N = 2
        x, res = LF.in_problem(N, Cw, H, W)
        xg = _guard((N, H, W, Cw), F16, gpu, R.nhwc(x))
        st = _guard((N, Cw, 2), F32, gpu, before=64, after=64)
        ws = _guard((ops.in_stats_ws_floats(N, H * W, Cw),), F32, gpu, before=64, after=64)
        ops.in_stats_into(xg.t, N, H * W, Cw, st.t, ws.t)
        torch.cuda.synchronize()
        what = "C%d %dx%d" % (Cw, H, W)
        s, sb, q, qb = R.in_stats_ref(x)
        worst_s = max(worst_s, _check(st.t[..., 0].double().cpu(), s, sb, "in_stats sum " + what),
                      _check(st.t[..., 1].double().cpu(), q, qb, "in_stats sumsq " + what))
        for gd in (xg, st, ws):
            gd.assert_untouched("in_stats " + what)
        # image 1 alone: the same bits
        st1 = torch.empty((1, Cw, 2), dtype=F32, device=gpu)
        ops.in_stats_into(xg.t[1:2].contiguous(), 1, H * W, Cw, st1)
        assert torch.equal(st1[0], st.t[1]), "in_stats %s: image 1 alone differs from image 1 of two" % what
        stats = st.t.cpu()
        small = H * W <= 1024
        combos = [(0, False), (1, False), (0, True), (1, True)] if small else [(1, False), (0, True)]
        for pad in (0, 1, 3):
            if min(H, W) <= pad:
                continue
            for relu, with_res in combos:
                rp = 1 if min(H, W) > 1 else 0
                rg = _guard((N, H + 2 * rp, W + 2 * rp, Cw), F16, gpu, R.nhwc(R.reflect_pad(res.float(), rp).half() if rp else res)) \
                    if with_res else None
                out = _guard((N, H + 2 * pad, W + 2 * pad, Cw), F16, gpu)
                flag = torch.zeros(64, dtype=torch.int32, device=gpu)
                ops.in_apply_into(xg.t, st.t, N, H, W, Cw, out.t, pad=pad, relu=relu, res=rg.t if with_res else None, res_pad=rp, flag=flag)
                torch.cuda.synchronize()
                w2 = "in_apply %s pad%d relu%d res%d" % (what, pad, relu, int(with_res))
                got = out.t.cpu()
                inner = got[:, pad:pad + H, pad:pad + W]
                ref, bound = R.in_apply_ref(x, stats, relu, res if with_res else None)
                worst_a = max(worst_a, _check(_nchw(inner), ref, bound, w2))
                if pad:        # the borders are copies of the interior
                    want = R.reflect_pad(inner.permute(0, 3, 1, 2).float(), pad).permute(0, 2, 3, 1).half()
                    assert torch.equal(got, want), "%s: %d border elements are not the reflected interior" % (w2, int((got != want).sum()))
                alone = torch.empty((1, H + 2 * pad, W + 2 * pad, Cw), dtype=F16, device=gpu)
                ops.in_apply_into(xg.t[1:2].contiguous(), st.t[1:2].contiguous(), 1, H, W, Cw, alone, pad=pad, relu=relu,
                                  res=rg.t[1:2].contiguous() if with_res else None, res_pad=rp)
                assert torch.equal(alone[0].cpu(), got[1]), w2 + ": image 1 alone differs"
                assert int(flag[0]) == 0
                for gd in (xg, st, out) + ((rg,) if with_res else ()):
                    gd.assert_untouched(w2)
    print("PARITY lineart InstanceNorm C%d: worst stats |err| / bound %.3f, worst apply |err| / bound %.3f" % (Cw, worst_s, worst_a))


def test_instance_norm_equals_torchs(ops, gpu):
    """statistics + apply against F.instance_norm on the fp16 values (biased variance, eps 1e-5), one fp16 store apart"""
    x, _ = LF.in_problem(2, 128, 23, 29)
    xd = R.nhwc(x).to(gpu)
    st = torch.empty((2, 128, 2), dtype=F32, device=gpu)
    out = torch.empty((2, 23, 29, 128), dtype=F16, device=gpu)
    ops.in_stats_into(xd, 2, 23 * 29, 128, st)
    ops.in_apply_into(xd, st, 2, 23, 29, 128, out)
    want = F.instance_norm(x.double(), eps=1e-5)
    err = (_nchw(out) - want).abs()
    assert bool((err <= 2.0 ** -10 * want.abs() + 1e-5).all()), float(err.max())


def test_apply_raises_the_range_flag(ops, gpu):
    x = torch.full((1, 4, 4, 64), 1000.0, dtype=F16, device=gpu)
    res = torch.full((1, 4, 4, 64), 65000.0, dtype=F16, device=gpu)
    st = torch.zeros((1, 64, 2), dtype=F32, device=gpu)
    st[..., 1] = 16.0                                  # mean 0, variance 1: y = 1000 + 65000
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    out = torch.empty((1, 4, 4, 64), dtype=F16, device=gpu)
    ops.in_apply_into(x, st, 1, 4, 4, 64, out, res=res, res_pad=0, flag=flag)
    torch.cuda.synchronize()
    assert int(flag[0]) == 1


# ---------------------------------------------------------------------------------------------------------------- the two GEMM forms
@pytest.mark.parametrize("Ci,Co", LF.CONVT_WIDTHS)
def test_transposed_conv_as_phase_form(ops, gpu, Ci, Co):
    for N in LF.BATCHES:
        for H, W in LF.CONVT_SIZES:
            x, w = LF.conv_problem(N, Ci, Co, H, W, transposed=True)
            wp = ops.pack_convT_w_phase(w.float().to(gpu))
            assert torch.equal(wp.cpu().reshape(4, Co, 4, Ci), R.pack_convT_phase(w)), "the packer differs from the restated pack"
            xg = _guard((N, H, W, Ci), F16, gpu, R.nhwc(x))
            out = _guard((N, 2 * H, 2 * W, Co), F16, gpu)
            ops.igemm(xg.t, Ci, wp, N * 4 * H * W, Co, Ci, taps=4, mode=ops.IG_CONV2D_PHASE,
                      geom=dict(Hin=H, Win=W, Hout=2 * H, Wout=2 * W, stride=1, up=2), rows_per_img=4 * H * W,
                      segs=[(out.t, Co, 0, Co, ops.SEG_ROW, 1)])
            torch.cuda.synchronize()
            ref, mag = R.convT_ref(x, w)
            what = "convT %d->%d N%d %dx%d" % (Ci, Co, N, H, W)
            helpers.assert_igemm_close(_nchw(out.t), ref, mag, 4 * Ci, 1.0, what, out_dtype=F16)
            xg.assert_untouched(what)
            out.assert_untouched(what)


def test_convT_packer_flags_overflow_and_takes_every_dtype(ops, gpu):
    _, w = LF.conv_problem(1, 64, 64, 1, 1, transposed=True)
    want = R.pack_convT_phase(w)
    for dt in (F32, F16, torch.bfloat16):
        src = w.to(dt)
        assert torch.equal(ops.pack_convT_w_phase(src.to(gpu)).cpu().reshape(4, 64, 4, 64), R.pack_convT_phase(src.float()).half())
    ovf = torch.zeros(4, dtype=torch.int32, device=gpu)
    ops.pack_convT_w_phase(w.float().to(gpu), ovf=ovf)
    assert int(ovf[0]) == 0 and want.dtype == F16
    big = w.float().clone()
    big[3, 5, 0, 2] = 1e5
    ops.pack_convT_w_phase(big.to(gpu), ovf=ovf)
    assert int(ovf[0]) == 1


@pytest.mark.parametrize("wide", [0, 2])
def test_valid_conv_over_padded_operand(ops, gpu, wide):
    """tap_origin = 1, stride 1, Hin = Hout + 2: the form of the residual blocks, in the ring kernels (wide 0) and the 8-phase kernel (2)"""
    seen = set()
    ops.set_igemm_wide(wide)
    try:
        for N, H, W in LF.valid_conv_cases():
            xp, w = LF.conv_problem(N, 256, 256, H + 2, W + 2)          # any padded map: the form does not care what the border holds
            xg = _guard((N, H + 2, W + 2, 256), F16, gpu, R.nhwc(xp))
            wg = _guard((256, 9 * 256), F16, gpu, R.pack_conv(w))
            out = _guard((N, H, W, 256), F16, gpu)
            kw = dict(A=xg.t, lda=256, W=wg.t, M=N * H * W, Nout=256, Cin=256, taps=9, mode=ops.IG_CONV2D,
                      geom=dict(Hin=H + 2, Win=W + 2, Hout=H, Wout=W, stride=1, up=1), rows_per_img=H * W, tap_origin=1,
                      segs=[(out.t, 256, 0, 256, ops.SEG_ROW, 1)])
            seen.add(ops.igemm_select(ops.igemm_desc(**kw)).split("<")[0])
            ops.igemm(**kw)
            torch.cuda.synchronize()
            ref, mag = R.conv_valid_ref(xp, w)
            what = "valid 3x3 wide%d N%d %dx%d (M %d)" % (wide, N, H, W, N * H * W)
            helpers.assert_igemm_close(_nchw(out.t), ref, mag, 9 * 256, 1.0, what, out_dtype=F16)
            for gd in (xg, wg, out):
                gd.assert_untouched(what)
    finally:
        ops.set_igemm_wide(-1)
    print("LINEART valid 3x3, wide %d: kernels %s" % (wide, sorted(seen)))
    assert ("igemm8_kernel" in seen) == (wide == 2)


# ---------------------------------------------------------------------------------------------------------------- plan == its parts
def _chain_by_hand(ops, gpu, sd, frames, ch):
    """the forward as op calls with the weights packed here -> (uint8, logits)"""
    N, H, W = frames.shape[:3]
    h2, w2, h, w = H // 2, W // 2, H // 4, W // 4
    dev = lambda t: t.to(gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    f16 = lambda *s: torch.empty(s, dtype=F16, device=gpu)
    st = torch.empty((N, 256, 2), dtype=F32, device=gpu)

    def norm(x, hh, ww, Cw, relu, pad, res=None):
        y = f16(N, hh + 2 * pad, ww + 2 * pad, Cw)
        ops.in_stats_into(x, N, hh * ww, Cw, st)
        ops.in_apply_into(x, st, N, hh, ww, Cw, y, pad=pad, relu=relu, res=res, res_pad=1, flag=flag)
        return y

    def conv(x, key, Ci, Co, hin, win, ho, wo, stride, origin):
        y = f16(N, ho, wo, Co)
        wp = ops.pack_conv_w(dev(sd[key + ".weight"]))
        ops.igemm(x, Ci, wp, N * ho * wo, Co, Ci, taps=9, mode=ops.IG_CONV2D, geom=dict(Hin=hin, Win=win, Hout=ho, Wout=wo, stride=stride, up=1),
                  rows_per_img=ho * wo, tap_origin=origin, segs=[(y, Co, 0, Co, ops.SEG_ROW, 1)])
        return y

    def convT(x, key, Ci, Co, hin, win):
        y = f16(N, 2 * hin, 2 * win, Co)
        wp = ops.pack_convT_w_phase(dev(sd[key + ".weight"]))
        ops.igemm(x, Ci, wp, N * 4 * hin * win, Co, Ci, taps=4, mode=ops.IG_CONV2D_PHASE,
                  geom=dict(Hin=hin, Win=win, Hout=2 * hin, Wout=2 * win, stride=1, up=2), rows_per_img=4 * hin * win,
                  segs=[(y, Co, 0, Co, ops.SEG_ROW, 1)])
        return y

    t = f16(N, H, W, 64)
    ops.lineart_stem_into(dev(frames), dev(R.pack_stem(sd["model0.1.weight"])), t, flag)
    x = norm(t, H, W, 64, True, 0)
    x = norm(conv(x, "model1.0", 64, 128, H, W, h2, w2, 2, 0), h2, w2, 128, True, 0)
    x = norm(conv(x, "model1.3", 128, 256, h2, w2, h, w, 2, 0), h, w, 256, True, 1)
    for b in range(3):
        y = norm(conv(x, "model2.%d.conv_block.1" % b, 256, 256, h + 2, w + 2, h, w, 1, 1), h, w, 256, True, 1)
        x = norm(conv(y, "model2.%d.conv_block.5" % b, 256, 256, h + 2, w + 2, h, w, 1, 1), h, w, 256, False, 1 if b < 2 else 0, res=x)
    x = norm(convT(x, "model3.0", 256, 128, h, w), h2, w2, 128, True, 0)
    x = norm(convT(x, "model3.3", 128, 64, h2, w2), H, W, 64, True, 3)
    out = torch.empty((N, H, W, 3) if ch == 3 else (N, H, W), dtype=U8, device=gpu)
    lg = torch.empty((N, H, W), dtype=F32, device=gpu)
    ops.lineart_head_into(x, N, H, W, dev(R.pack_head(sd["model4.1.weight"])), float(sd["model4.1.bias"][0]), out, lg)
    torch.cuda.synchronize()
    assert int(flag[0]) == 0
    return out, lg


@pytest.mark.parametrize("H,W", LF.PLAN_SIZES)
def test_plan_equals_its_parts(ops, gpu, H, W):
    import ctrl_adapter_amd as P
    fine, coarse = R.make_state_dict(31, "calibrated"), R.make_state_dict(32, "calibrated")
    frames = R.make_frames(9, 2, H, W)
    det = P.LineartDetector.from_state_dict(fine, coarse, device=gpu)
    for is_coarse, sd in ((False, fine), (True, coarse)):
        out, lg = det.run(frames.to(gpu), coarse=is_coarse, return_logits=True)
        want, wl = _chain_by_hand(ops, gpu, sd, frames, 3)
        assert torch.equal(lg, wl), "coarse=%s: %d logits differ between the plan and its kernels chained by hand" % (is_coarse, int((lg != wl).sum()))
        assert torch.equal(out, want)
        assert float(lg.std()) > 0.5
    assert not torch.equal(det.run(frames.to(gpu)), det.run(frames.to(gpu), coarse=True))
    with pytest.raises(ValueError, match="coarse"):
        P.LineartDetector.from_state_dict(fine, device=gpu).run(frames.to(gpu), coarse=True)


# ---------------------------------------------------------------------------------------------------------------- the whole detector
@pytest.mark.parametrize("key", list(LF.DETECTOR_CASES))
def test_detector_against_fp64(gpu, key):
    """every logit within 4 x max |emulated - fp64| of the fp64 restatement; the bytes inside what that tolerance allows"""
    import ctrl_adapter_amd as P
    N, H, W = LF.DETECTOR_CASES[key]
    sd = R.make_state_dict(3, "calibrated")
    fr = R.make_frames(5, N, H, W)
    ref, emu, dev, tol = R.detector_tolerance(sd, fr)
    det = P.LineartDetector.from_state_dict(sd, device=gpu)
    soft, lg = det.run(fr.to(gpu), channels=1, return_logits=True)
    soft, lg = soft.cpu().numpy(), lg.double().cpu()
    worst = float((lg - ref).abs().max())
    n = R.outside(lg, ref, tol)
    nu = R.u8_failures(soft, ref.numpy(), np.full(ref.shape, tol))
    print("LINEART-DETECTOR %s: logit std %.3f | emulated deviation %.3e, tolerance %.3e, measured deviation %.3e (vs emulated: %.3e); "
          "%d logits, %d bytes outside" % (key, float(ref.std()), dev, tol, worst, float((lg - emu).abs().max()), n, nu))
    assert n == 0 and nu == 0
    assert len(np.unique(soft)) > 20
    three = det.run(fr.to(gpu), channels=3).cpu().numpy()
    assert np.array_equal(three[..., 0], soft) and np.array_equal(three[..., 1], soft) and np.array_equal(three[..., 2], soft)


def test_dropped_biases_do_not_matter(gpu):
    """two state dicts that differ only in the biases in front of an InstanceNorm: bit-identical maps, and the fp64 restatement, which keeps
    the biases, stays inside the tolerance"""
    import ctrl_adapter_amd as P
    a, b = R.make_state_dict(3, "calibrated"), R.make_state_dict(3, "calibrated", bias_seed=8)
    assert not torch.equal(a["model2.0.conv_block.1.bias"], b["model2.0.conv_block.1.bias"]) and torch.equal(a["model4.1.bias"], b["model4.1.bias"])
    fr = R.make_frames(5, 1, 64, 64)
    oa, la = P.LineartDetector.from_state_dict(a, device=gpu).run(fr.to(gpu), return_logits=True)
    ob, lb = P.LineartDetector.from_state_dict(b, device=gpu).run(fr.to(gpu), return_logits=True)
    assert torch.equal(la, lb) and torch.equal(oa, ob)
    ref, emu, dev, tol = R.detector_tolerance(b, fr)
    n = R.outside(lb.double().cpu(), ref, tol)
    print("LINEART-BIASES: measured deviation %.3e against the restatement WITH biases, tolerance %.3e, %d outside" % (
        float((lb.double().cpu() - ref).abs().max()), tol, n))
    assert n == 0


def test_frames_do_not_depend_on_batch_or_group(gpu):
    import ctrl_adapter_amd as P
    det = P.LineartDetector.from_state_dict(R.make_state_dict(31, "calibrated"), device=gpu)
    frames = R.make_frames(9, 3, 64, 128).to(gpu)
    whole, wl = det.run(frames, return_logits=True)
    assert float(wl.std()) > 0.5
    alone, al = det.run(frames[1:2], return_logits=True)
    assert torch.equal(al[0], wl[1]), "frame 1: %d logits differ between N = 1 and N = 3" % int((al[0] != wl[1]).sum())
    assert torch.equal(alone[0], whole[1])
    for fpg in (1, 2):
        again, gl = det.run(frames, return_logits=True, frames_per_group=fpg)
        assert torch.equal(gl, wl) and torch.equal(again, whole), "frames_per_group=%d: %d logits differ" % (fpg, int((gl != wl).sum()))
    assert det.workspace_bytes(3, 64, 128, frames_per_group=1) < det.workspace_bytes(3, 64, 128, frames_per_group=2) \
        < det.workspace_bytes(3, 64, 128, frames_per_group=3) <= det.workspace_bytes(3, 64, 128)
    assert det.workspace_bytes(3, 64, 96) == 0 and det.workspace_bytes(0, 64, 64) == 0
    capped = P.LineartDetector.from_state_dict(R.make_state_dict(31, "calibrated"), device=gpu, ws_cap_bytes=det.workspace_bytes(1, 64, 128) + 4096)
    assert capped.workspace_bytes(3, 64, 128) == det.workspace_bytes(3, 64, 128, frames_per_group=1)
    assert torch.equal(capped.run(frames), whole)


def test_tall_frames_do_not_depend_on_batch_or_group(gpu):
    import ctrl_adapter_amd as P
    det = P.LineartDetector.from_state_dict(R.make_state_dict(31, "calibrated"), device=gpu)
    frames = R.make_frames(11, 3, 128, 64).to(gpu)
    whole, wl = det.run(frames, return_logits=True)
    alone, al = det.run(frames[1:2], return_logits=True)
    assert torch.equal(al[0], wl[1]) and torch.equal(alone[0], whole[1])
    again, gl = det.run(frames, return_logits=True, frames_per_group=1)
    assert torch.equal(gl, wl) and torch.equal(again, whole)


def test_range_guard(gpu):
    """a checkpoint scaled so that the stem leaves the fp16 range: the forward says so, and the next clean forward runs"""
    import ctrl_adapter_amd as P
    frames = R.make_frames(9, 1, 64, 64).to(gpu)
    det = P.LineartDetector.from_state_dict(R.make_state_dict(31, "calibrated", gain=2.0 ** 22), device=gpu)
    with pytest.raises(RuntimeError, match="fp16 range"):
        det.run(frames)
    ok = P.LineartDetector.from_state_dict(R.make_state_dict(31, "calibrated"), device=gpu)
    out, lg = ok.run(frames, return_logits=True)
    assert bool(torch.isfinite(lg).all()) and out.shape == (1, 64, 64, 3)
    with pytest.raises(RuntimeError, match="fp16 range"):
        det.run(frames)
    assert torch.equal(ok.run(frames), out)


def test_extract_lineart_feeds_prepare_images(gpu):
    """raw frames -> the lineart map -> controlnet_cond without leaving the device"""
    import ctrl_adapter_amd as P
    from oracle import image_prep as O
    from PIL import Image
    det = P.LineartDetector.from_state_dict(R.make_state_dict(3, "calibrated"), R.make_state_dict(4, "calibrated"), device=gpu).to("cuda")
    frames = R.make_frames(9, 2, 64, 64).numpy()
    cond = P.extract_lineart([Image.fromarray(frames[0]), frames[1]], det)
    assert cond.dtype == U8 and cond.shape == (2, 64, 64, 3) and cond.is_cuda and cond.is_contiguous() and len(torch.unique(cond)) > 20
    assert torch.equal(cond, det(list(frames), detect_resolution=64, image_resolution=64, output_type="pt"))
    assert not torch.equal(cond, P.extract_lineart(list(frames), det, coarse=True))
    pil = P.extract_lineart(list(frames), det, as_pil=True)
    assert np.array_equal(np.asarray(pil[1]), cond[1].cpu().numpy())
    one = det(frames[0], detect_resolution=64, image_resolution=64, output_type="np")
    assert np.array_equal(one, cond[0].cpu().numpy())
    got = P.prepare_images(list(cond), 64, 64, 1, 1, gpu, torch.float16, do_classifier_free_guidance=True)
    want = O.prepare_images([c.cpu().numpy() for c in cond], 64, 64, 1, 1, dtype=torch.float16, do_classifier_free_guidance=True)
    assert got.shape == want.shape == (2, 2, 3, 64, 64) and got.dtype == want.dtype
    assert torch.equal(got.cpu(), want), "%d differing elements" % int((got.cpu() != want).sum())
