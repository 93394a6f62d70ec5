"""The PiDiNet annotator on the GPU (csrc/pidinet.hip, csrc/plan_pidinet.cpp, ctrl_adapter_amd.pidinet) against tests/pidinet_ref.py.

Kernel forms, each inside poisoned surroundings and against its fp64 reference with the element-wise bound of pidinet_ref (nothing is
measured, there is no slack factor): the stem, every (kind, width, skip) form of the fused PDC block at the tile edges that
ctrl_pidi_launch_shape reports, the context head (reduce, context, side map) and the fuse.  The plan is bit-identical to its kernels
chained by hand, so nothing between the kernels goes unchecked.  The whole detector on the calibrated checkpoint: every logit within
4 x max |emulated - fp64| of the fp64 restatement (the tolerance tests/test_pidinet_host.py proves every planted error against).
Figures are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import annot_forms as AF
import hed_ref as HR
import helpers
import pidinet_forms as PF
import pidinet_ref as R
from helpers import Guarded

pytestmark = pytest.mark.gpu
U8, F16, F32 = torch.uint8, torch.float16, torch.float32
U8_POISON = 0xA5
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def lib(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def tiles(lib):
    out = []
    for k in (0, 1):
        th, tw = C.c_int(), C.c_int()
        assert lib.ctrl_pidi_launch_shape(k, C.byref(th), C.byref(tw)) == 0
        out.append((th.value, tw.value))
    return out


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.ctrl_last_error().decode()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


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
        g.view.copy_(torch.as_tensor(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data).reshape(-1).to(dtype))
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
    print("PIDI-CHECK %-58s worst err/bound %.3f  rel_inf %.2e" % (what, worst, float(err.max() / ref.abs().max().clamp_min(1e-12))))
    bad = err > bound
    assert not bool(bad.any()), "%s: %d of %d elements beyond the bound (worst %.2f); first at %s" % (
        what, int(bad.sum()), bad.numel(), worst, tuple(int(v) for v in bad.nonzero()[0]))
    return worst


def _nchw(t_nhwc, C_):
    return t_nhwc[..., :C_].permute(0, 3, 1, 2).double().cpu()


# ---------------------------------------------------------------------------------------------------------------- stem
def test_stem_channel_order_and_padding(lib, gpu):
    """a frame whose three channels differ: only BGR / 255 against the converted cd kernel stays inside the bound; pad channels are zero"""
    N, H, W = 2, 64, 72
    fr = R.make_frames(7, N, H, W)
    fr[..., 0] = fr[..., 0] // 3                     # red dark, blue bright: a swapped order moves every output
    fr[..., 2] = 255 - fr[..., 2] // 4
    fr[0, 0, 0] = torch.tensor([255, 0, 128], dtype=U8)
    w = R.make_state_dict(21, "he")["init_block.weight"] * 4
    kern = PF.lib_convert("cd", w)
    src = _guard((N, H, W, 3), U8, gpu, fr)
    wp = _guard((27 * 64,), F32, gpu, R.pack_stem(kern))
    out = _guard((N, H, W, 64), F16, gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    _ok(lib, lib.ctrl_op_pidi_stem(_ptr(src.t), N, H, W, _ptr(wp.t), _ptr(out.t), _ptr(flag), _stream()))
    torch.cuda.synchronize()
    ref, bound = R.stem_ref(fr, kern)
    _check(_nchw(out.t, 60), ref, bound, "stem %dx%dx%d" % (N, H, W))
    swapped, _ = R.stem_ref(fr.flip(-1), kern)
    assert int(((swapped - ref).abs() > bound).sum()) > ref.numel() // 2          # the check tells the orders apart
    assert bool((out.t[..., 60:] == 0).all()) and int(flag[0]) == 0
    for gd in (src, wp, out):
        gd.assert_untouched("stem")


def test_stem_forms(lib, gpu):
    """annot_forms.STEM_SIZES: a ragged last workgroup behind full ones and alone, one quad per row, H < 3, a tall frame, corner pixels 255
    and 0; stem_ref's bound unchanged"""
    worst = 0.0
    for N, H, W in AF.STEM_SIZES:
        fr, kern, ref, bound = AF.pidi_stem_problem(N, H, W)
        src = _guard((N, H, W, 3), U8, gpu, fr)
        wp = _guard((27 * 64,), F32, gpu, R.pack_stem(kern))
        out = _guard((N, H, W, 64), F16, gpu)
        flag = torch.zeros(64, dtype=torch.int32, device=gpu)
        _ok(lib, lib.ctrl_op_pidi_stem(_ptr(src.t), N, H, W, _ptr(wp.t), _ptr(out.t), _ptr(flag), _stream()))
        torch.cuda.synchronize()
        worst = max(worst, _check(_nchw(out.t, 60), ref, bound, "stem %dx%dx%d" % (N, H, W)))
        assert bool((out.t[..., 60:] == 0).all()) and int(flag[0]) == 0
        for gd in (src, wp, out):
            gd.assert_untouched("stem %dx%dx%d" % (N, H, W))
    print("PARITY pidi stem: worst |err| / bound %.3f over %d sizes" % (worst, len(AF.STEM_SIZES)))


# ---------------------------------------------------------------------------------------------------------------- PDC block
def _run_block(lib, gpu, x_nhwc, N, H, W, cin, cout, taps, dw, w2, wsc, bsc, pool, flag):
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    xg = _guard(tuple(x_nhwc.shape), F16, gpu, x_nhwc)
    out = _guard((N, Ho, Wo, R.cp(cout)), F16, gpu)
    _ok(lib, lib.ctrl_op_pidi_block(_ptr(xg.t), N, H, W, cin, cout, taps, _ptr(dw.t), _ptr(w2.t), _ptr(wsc.t if wsc else None),
                                    _ptr(bsc.t if bsc else None), int(pool), _ptr(out.t), _ptr(flag), _stream()))
    torch.cuda.synchronize()
    xg.assert_untouched("block x")
    out.assert_untouched("block out")
    return out.t


@pytest.mark.parametrize("kind,cin,cout,pool", PF.block_forms(), ids=lambda v: str(v))
def test_block_form(lib, gpu, tiles, kind, cin, cout, pool):
    th, tw = tiles[0]
    taps = 25 if kind == "rd" else 9
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    for N in PF.BATCHES:
        for Ho, Wo in PF.block_sizes(th, tw):
            x, w1, w2, wsc, bsc = PF.block_problem(kind, cin, cout, pool, N, Ho, Wo, seed=cin + Ho + N)
            H, W = x.shape[2:]
            kern = PF.lib_convert(kind, w1)
            dw = _guard((taps * R.cp(cin),), F32, gpu, R.pack_dw(kern), before=64, after=64)
            w2g = _guard((R.cp(cout) * R.cp(cin),), F16, gpu, R.pack_1x1(w2))
            wsg = _guard((R.cp(cout) * R.cp(cin),), F16, gpu, R.pack_1x1(wsc)) if pool else None
            bsg = _guard((R.cp(cout),), F32, gpu, R.pack_vec(bsc, R.cp(cout)), before=64, after=64) if pool else None
            xp = R.pad_nhwc(x)
            got = _run_block(lib, gpu, xp, N, H, W, cin, cout, taps, dw, w2g, wsg, bsg, pool, flag)
            ref, bound = R.block_ref(x, kern, w2, wsc, bsc, pool)
            _check(_nchw(got, cout), ref, bound, "block %s %d->%d%s N%d %dx%d" % (kind, cin, cout, " pool" if pool else "", N, Ho, Wo))
            assert bool((got[..., cout:] == 0).all()), "pad channels of the output are not exact zeros"
            xp[..., cin:] = PF.PAD_GARBAGE
            again = _run_block(lib, gpu, xp, N, H, W, cin, cout, taps, dw, w2g, wsg, bsg, pool, flag)
            assert torch.equal(again, got), "finite garbage in the input's pad channels changed %d outputs" % int((again != got).sum())
            for gd in (dw, w2g) + ((wsg, bsg) if pool else ()):
                gd.assert_untouched("block weights")
    assert int(flag[0]) == 0


def test_block_raises_the_range_flag(lib, gpu):
    x, w1, w2, _, _ = PF.block_problem("cv", 60, 60, False, 1, 8, 16, seed=1)
    x = (x.float() * 2.0 ** 14).half()
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    dw = _guard((9 * 64,), F32, gpu, R.pack_dw(PF.lib_convert("cv", w1)), before=64, after=64)
    w2g = _guard((64 * 64,), F16, gpu, R.pack_1x1(w2))
    _run_block(lib, gpu, R.pad_nhwc(x), 1, 8, 16, 60, 60, 9, dw, w2g, None, None, False, flag)
    assert int(flag[0]) == 1


# ---------------------------------------------------------------------------------------------------------------- context head
@pytest.mark.parametrize("Cw", PF.HEAD_WIDTHS)
def test_head(lib, gpu, tiles, Cw):
    """reduce -> context -> side map, every stage against its own reference on the inputs the GPU produced"""
    for N, (H, W) in zip((2, 1, 3), PF.head_sizes(tiles[1][0])):
        x, w1, b1, ws, att_w, att_b, red_w, side_w, red_b = PF.head_problem(Cw, N, H, W, seed=Cw + H)
        xp = R.pad_nhwc(x)
        xp[..., Cw:] = PF.PAD_GARBAGE
        xg = _guard(tuple(xp.shape), F16, gpu, xp)
        w1g = _guard((32 * R.cp(Cw),), F16, gpu, R.pack_1x1(w1, 32))
        b1g = _guard((32,), F32, gpu, R.pack_vec(b1, 32), before=64, after=64)
        t = _guard((N, H, W, 32), F16, gpu)
        flag = torch.zeros(64, dtype=torch.int32, device=gpu)
        _ok(lib, lib.ctrl_op_pidi_head_reduce(_ptr(xg.t), N, H, W, Cw, _ptr(w1g.t), _ptr(b1g.t), _ptr(t.t), _ptr(flag), _stream()))
        torch.cuda.synchronize()
        what = "C%d N%d %dx%d" % (Cw, N, H, W)
        ref, bound = R.head_reduce_ref(x, w1, b1)
        _check(_nchw(t.t, R.DIL), ref, bound, "head reduce " + what)
        assert bool((t.t[..., R.DIL:] == 0).all()) and int(flag[0]) == 0
        wdg = _guard((36 * 32 * 32,), F16, gpu, R.pack_dilated(ws))
        par = torch.cat([att_w.reshape(-1), att_b, red_w.reshape(-1)])
        a4 = _guard((N, H, W, 4), F32, gpu)
        d = _guard((N, H, W), F32, gpu)
        _ok(lib, lib.ctrl_op_pidi_head_context(_ptr(t.t), N, H, W, _ptr(wdg.t), _floats(par), _ptr(a4.t), _ptr(d.t), _stream()))
        torch.cuda.synchronize()
        t16 = t.t[..., :R.DIL].permute(0, 3, 1, 2).cpu()
        ra, ba, rd, bd = R.head_context_ref(t16, ws, att_w, att_b, red_w)
        _check(a4.t.permute(0, 3, 1, 2).double().cpu(), ra, ba, "head context a4 " + what)
        _check(d.t[:, None].double().cpu(), rd, bd, "head context d " + what)
        e = _guard((N, H, W), F32, gpu)
        sp = torch.cat([side_w.reshape(4, 9).t().reshape(-1), red_b])
        _ok(lib, lib.ctrl_op_pidi_side(_ptr(a4.t), _ptr(d.t), N, H, W, _floats(sp), _ptr(e.t), _stream()))
        torch.cuda.synchronize()
        re, be = R.side_ref(a4.t.permute(0, 3, 1, 2).cpu(), d.t[:, None].cpu(), side_w, red_b)
        _check(e.t[:, None].double().cpu(), re, be, "side map " + what)
        for gd in (xg, w1g, b1g, t, wdg, a4, d, e):
            gd.assert_untouched("head " + what)


# ---------------------------------------------------------------------------------------------------------------- side map and fuse
def _side_and_fuse(lib, gpu, H, W, ch, filt):
    """-> (worst side |err| / bound, worst fuse logit |err| / bound)"""
    N = AF.PIDI_FUSE_N
    shares = [0.0, 0.0]
    g = torch.Generator().manual_seed(H + W + ch)
    cw, cb = [0.6, -0.5, 0.4, 0.5], 0.1
    es, refs = [], []
    for k in range(4):
        h, w = H >> k, W >> k
        a4 = _guard((N, h, w, 4), F32, gpu, torch.randn((N, h, w, 4), generator=g))
        d = _guard((N, h, w), F32, gpu, torch.randn((N, h, w), generator=g) * 2)
        sw, rb = torch.randn((1, 4, 3, 3), generator=g) / 2, torch.randn(1, generator=g) * 0.3
        e = _guard((N, h, w), F32, gpu, before=64, after=64)
        _ok(lib, lib.ctrl_op_pidi_side(_ptr(a4.t), _ptr(d.t), N, h, w, _floats(torch.cat([sw.reshape(4, 9).t().reshape(-1), rb])), _ptr(e.t),
                                       _stream()))
        torch.cuda.synchronize()
        re, be = R.side_ref(a4.t.permute(0, 3, 1, 2).cpu(), d.t[:, None].cpu(), sw, rb)
        shares[0] = max(shares[0], _check(e.t[:, None].double().cpu(), re, be, "side map stride %d of %dx%d" % (1 << k, H, W)))
        for gd in (a4, d, e):
            gd.assert_untouched("side")
        es.append(e)
    out = _guard((N, H, W) if ch == 1 else (N, H, W, 3), U8, gpu, before=96, after=96)
    lg = _guard((N, H, W), F32, gpu)
    arr = (C.c_void_p * 4)(*[e.t.data_ptr() for e in es])
    _ok(lib, lib.ctrl_op_pidi_fuse(arr, N, H, W, _floats(cw + [cb]), filt, ch, _ptr(out.t), _ptr(lg.t), _stream()))
    torch.cuda.synchronize()
    ref, bound = R.fuse_ref([e.t.cpu() for e in es], cw, cb, H, W)
    shares[1] = _check(lg.t.double().cpu(), ref, bound, "fuse logits %dx%d ch%d filter %d" % (H, W, ch, filt))
    got = out.t.cpu().numpy()
    first = got if ch == 1 else got[..., 0]
    ref, bound = ref.numpy(), bound.numpy()
    if filt:
        sure = np.abs(ref) > bound
        bad = int(((first != np.where(ref > 0, 255, 0)) & sure).sum())
        assert set(np.unique(first)) <= {0, 255} and int(sure.sum()) > ref.size * 0.99
    else:
        bad = HR.u8_failures(first, ref, bound)
        assert len(np.unique(first)) > min(50, first.size // 8)          # (50 for the 8192 bytes and more of FUSE_SIZES; a 2 x 8 x 8 map has 128)
    print("PIDI-FUSE %dx%d ch%d filter %d: %d bytes outside what the logit's bound allows" % (H, W, ch, filt, bad))
    assert bad == 0
    if ch == 3:
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    for gd in es + [out, lg]:
        gd.assert_untouched("fuse")
    return tuple(shares)


@pytest.mark.parametrize("H,W", PF.FUSE_SIZES)
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("filt", [0, 1])
def test_side_and_fuse(lib, gpu, H, W, ch, filt):
    _side_and_fuse(lib, gpu, H, W, ch, filt)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("filt", [0, 1])
def test_side_and_fuse_forms(lib, gpu, ch, filt):
    """annot_forms.PIDI_FUSE_SIZES: side maps down to 1 x 1, 1 x 3 and 3 x 1 (every tap but the centre outside; both clamps of torch_coord on
    one sample), H > W, a ragged last workgroup of both kernels behind full ones"""
    side = fuse = 0.0
    for H, W in AF.PIDI_FUSE_SIZES:
        a, b = _side_and_fuse(lib, gpu, H, W, ch, filt)
        side, fuse = max(side, a), max(fuse, b)
    print("PARITY pidi side: worst |err| / bound %.3f; pidi fuse<%d> filter %d: worst logit |err| / bound %.3f" % (side, ch, filt, fuse))


# ---------------------------------------------------------------------------------------------------------------- plan == its parts
def _chain_by_hand(lib, gpu, sd, frames, ch):
    """the forward as ctrl_op_pidi_* calls with the weights packed here -> (uint8, logits)"""
    N, H, W = frames.shape[:3]
    dev = lambda t: t.to(gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    x = torch.empty((N, H, W, 64), dtype=F16, device=gpu)
    wst = dev(R.pack_stem(PF.lib_convert("cd", sd["init_block.weight"])))
    _ok(lib, lib.ctrl_op_pidi_stem(_ptr(dev(frames)), N, H, W, _ptr(wst), _ptr(x), _ptr(flag), _stream()))
    h, w, es, keep = H, W, [], []
    for L, s, j, kind, cin, c, pool in R.layers():
        pre = "block%d_%d." % (s, j)
        kern = PF.lib_convert(kind, sd[pre + "conv1.weight"])
        dw, w2 = dev(R.pack_dw(kern)), dev(R.pack_1x1(sd[pre + "conv2.weight"]))
        wsc = dev(R.pack_1x1(sd[pre + "shortcut.weight"])) if pool else None
        bsc = dev(R.pack_vec(sd[pre + "shortcut.bias"], R.cp(c))) if pool else None
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        y = torch.empty((N, ho, wo, R.cp(c)), dtype=F16, device=gpu)
        _ok(lib, lib.ctrl_op_pidi_block(_ptr(x), N, h, w, cin, c, kern.shape[-1] ** 2, _ptr(dw), _ptr(w2), _ptr(wsc), _ptr(bsc), int(pool), _ptr(y),
                                        _ptr(flag), _stream()))
        keep += [dw, w2, wsc, bsc, x]
        x, h, w = y, ho, wo
        if j == R.BLOCKS[s - 1]:
            i = s - 1
            w1 = dev(R.pack_1x1(sd["dilations.%d.conv1.weight" % i], 32))
            b1 = dev(R.pack_vec(sd["dilations.%d.conv1.bias" % i], 32))
            wd = dev(R.pack_dilated([sd["dilations.%d.conv2_%d.weight" % (i, k)] for k in range(1, 5)]))
            t = torch.empty((N, h, w, 32), dtype=F16, device=gpu)
            a4 = torch.empty((N, h, w, 4), dtype=F32, device=gpu)
            d = torch.empty((N, h, w), dtype=F32, device=gpu)
            e = torch.empty((N, h, w), dtype=F32, device=gpu)
            p124, p37 = R.head_par(sd, i)
            _ok(lib, lib.ctrl_op_pidi_head_reduce(_ptr(x), N, h, w, c, _ptr(w1), _ptr(b1), _ptr(t), _ptr(flag), _stream()))
            _ok(lib, lib.ctrl_op_pidi_head_context(_ptr(t), N, h, w, _ptr(wd), _floats(p124), _ptr(a4), _ptr(d), _stream()))
            _ok(lib, lib.ctrl_op_pidi_side(_ptr(a4), _ptr(d), N, h, w, _floats(p37), _ptr(e), _stream()))
            keep += [w1, b1, wd, t, a4, d]
            es.append(e)
    out = torch.empty((N, H, W, 3) if ch == 3 else (N, H, W), dtype=U8, device=gpu)
    lg = torch.empty((N, H, W), dtype=F32, device=gpu)
    arr = (C.c_void_p * 4)(*[e.data_ptr() for e in es])
    cls = [float(v) for v in sd["classifier.weight"].reshape(-1)] + [float(sd["classifier.bias"][0])]
    _ok(lib, lib.ctrl_op_pidi_fuse(arr, N, H, W, _floats(cls), 0, ch, _ptr(out), _ptr(lg), _stream()))
    torch.cuda.synchronize()
    assert int(flag[0]) == 0
    return out, lg


@pytest.mark.parametrize("H,W", PF.FUSE_SIZES)
def test_plan_equals_its_parts(lib, gpu, H, W):
    import ctrl_adapter_amd as P
    sd = R.make_state_dict(31, "he")
    frames = R.make_frames(9, 2, H, W)
    det = P.PidiNetDetector.from_state_dict(sd, device=gpu)
    out, lg = det.run(frames.to(gpu), return_logits=True)
    want, wl = _chain_by_hand(lib, gpu, sd, frames, 3)
    assert torch.equal(lg, wl), "%d logits differ between the plan and its kernels chained by hand" % int((lg != wl).sum())
    assert torch.equal(out, want)
    assert float(lg.std()) > 0.01


# ---------------------------------------------------------------------------------------------------------------- the whole detector
@pytest.fixture(scope="module")
def calibrated(gpu):
    sd = R.make_state_dict(3, "calibrated")
    cases = {}
    for key, (N, H, W) in PF.DETECTOR_CASES.items():
        fr = R.make_frames(5, N, H, W)
        cases[key] = (fr,) + R.detector_tolerance(sd, fr)
    return sd, cases


def test_detector_against_fp64(gpu, calibrated):
    """every logit within 4 x max |emulated - fp64| of the fp64 restatement; the bytes inside what that tolerance allows; the scribble output
    equal to the restated tail of the detector's own soft map"""
    import ctrl_adapter_amd as P
    sd, cases = calibrated
    det = P.PidiNetDetector.from_state_dict(sd, device=gpu)
    for key, (fr, ref, emu, dev, tol) in cases.items():
        soft, lg = det.run(fr.to(gpu), channels=1, return_logits=True)
        soft, lg = soft.cpu().numpy(), lg.double().cpu()
        worst = float((lg - ref).abs().max())
        n = R.outside(lg, ref, tol)
        nu = HR.u8_failures(soft, ref.numpy(), np.full(ref.shape, tol))
        print("PIDI-DETECTOR %s: logit std %.3f | emulated deviation %.3e, tolerance %.3e, measured deviation %.3e (vs emulated: %.3e); "
              "%d logits, %d bytes outside" % (key, float(ref.std()), dev, tol, worst, float((lg - emu).abs().max()), n, nu))
        assert n == 0 and nu == 0
        assert len(np.unique(soft)) > 20
        scr = det.run(fr.to(gpu), scribble=True, channels=3).cpu().numpy()
        for i in range(fr.shape[0]):
            want = HR.scribble_tail(soft[i])
            dd = HR.exact_failures(np.ascontiguousarray(scr[i][..., 0]), want)
            print("PARITY pidi scribble %s frame %d: %d of %d bytes differ; %d set" % (key, i, dd, want.size, int((want > 0).sum())))
            assert dd == 0
            assert np.array_equal(scr[i][..., 0], scr[i][..., 1]) and np.array_equal(scr[i][..., 0], scr[i][..., 2])
        filt = det.run(fr.to(gpu), apply_filter=True, channels=1).cpu().numpy()
        clear = np.abs(lg.numpy()) > 1e-6              # edge > 0.5 is logit > 0; logits that round to a sigmoid of 0.5 are left out
        assert set(np.unique(filt)) <= {0, 255} and np.array_equal(filt[clear] == 255, lg.numpy()[clear] > 0)


def test_frames_do_not_depend_on_batch_or_group(gpu):
    import ctrl_adapter_amd as P
    det = P.PidiNetDetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    frames = R.make_frames(9, 3, 64, 128).to(gpu)
    whole, wl = det.run(frames, return_logits=True)
    for n in range(3):
        alone, al = det.run(frames[n:n + 1], return_logits=True)
        assert torch.equal(al[0], wl[n]), "frame %d: %d logits differ between N = 1 and N = 3" % (n, int((al[0] != wl[n]).sum()))
        assert torch.equal(alone[0], whole[n])
    for fpg in (1, 2):
        again, gl = det.run(frames, return_logits=True, frames_per_group=fpg)
        assert torch.equal(gl, wl) and torch.equal(again, whole), "frames_per_group=%d: %d logits differ" % (fpg, int((gl != wl).sum()))
    scr = det.run(frames, scribble=True)
    assert torch.equal(det.run(frames, scribble=True, frames_per_group=1), scr) and torch.equal(det.run(frames[1:2], scribble=True)[0], scr[1])
    assert det.workspace_bytes(3, 64, 128, frames_per_group=1) < det.workspace_bytes(3, 64, 128, frames_per_group=2) \
        <= det.workspace_bytes(3, 64, 128)


def test_tall_frames_do_not_depend_on_batch_or_group(gpu):
    """128 x 64: two tile rows of every tiled kernel per frame"""
    import ctrl_adapter_amd as P
    det = P.PidiNetDetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    frames = R.make_frames(11, 3, 128, 64).to(gpu)
    whole, wl = det.run(frames, return_logits=True)
    assert float(wl.std()) > 0.01
    for n in range(3):
        alone, al = det.run(frames[n:n + 1], return_logits=True)
        assert torch.equal(al[0], wl[n]), "frame %d: %d logits differ between N = 1 and N = 3" % (n, int((al[0] != wl[n]).sum()))
        assert torch.equal(alone[0], whole[n])
    for fpg in (1, 2):
        again, gl = det.run(frames, return_logits=True, frames_per_group=fpg)
        assert torch.equal(gl, wl) and torch.equal(again, whole), "frames_per_group=%d: %d logits differ" % (fpg, int((gl != wl).sum()))
    scr = det.run(frames, scribble=True)
    assert torch.equal(det.run(frames, scribble=True, frames_per_group=1), scr) and torch.equal(det.run(frames[1:2], scribble=True)[0], scr[1])


def test_range_guard(gpu):
    """a checkpoint scaled so that the stem leaves the fp16 range: the forward says so"""
    import ctrl_adapter_amd as P
    frames = R.make_frames(9, 1, 64, 64).to(gpu)
    det = P.PidiNetDetector.from_state_dict(R.make_state_dict(31, "he", gain=2.0 ** 22), device=gpu)
    with pytest.raises(RuntimeError, match="fp16 range"):
        det.run(frames)
    ok = P.PidiNetDetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    out, lg = ok.run(frames, return_logits=True)
    assert bool(torch.isfinite(lg).all()) and out.shape == (1, 64, 64, 3)


def test_extract_softedge_feeds_prepare_images(gpu):
    """raw frames -> PiDiNet's soft-edge map -> controlnet_cond without leaving the device"""
    import ctrl_adapter_amd as P
    from oracle import image_prep as O
    from PIL import Image
    det = P.PidiNetDetector.from_state_dict(R.make_state_dict(3, "calibrated"), device=gpu)
    frames = R.make_frames(9, 2, 64, 64).numpy()
    cond = P.extract_softedge([Image.fromarray(frames[0]), frames[1]], det)
    assert cond.dtype == U8 and cond.shape == (2, 64, 64, 3) and cond.is_cuda and cond.is_contiguous() and len(torch.unique(cond)) > 20
    assert torch.equal(cond, det(list(frames), detect_resolution=64, image_resolution=64, output_type="pt"))
    scr = P.extract_scribble(list(frames), det)
    assert set(np.unique(scr.cpu().numpy())) <= {0, 255}
    pil = P.extract_softedge(list(frames), det, as_pil=True)
    assert np.array_equal(np.asarray(pil[1]), cond[1].cpu().numpy())
    got = P.prepare_images(list(cond), 64, 64, 1, 1, gpu, torch.float16, do_classifier_free_guidance=True)
    want = O.prepare_images([c.cpu().numpy() for c in cond], 64, 64, 1, 1, dtype=torch.float16, do_classifier_free_guidance=True)
    assert got.shape == want.shape == (2, 2, 3, 64, 64) and got.dtype == want.dtype
    assert torch.equal(got.cpu(), want), "%d differing elements" % int((got.cpu() != want).sum())
