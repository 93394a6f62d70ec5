"""The HED annotator on the GPU (csrc/hed.hip, csrc/plan_hed.cpp, ctrl_adapter_amd.hed) against tests/hed_ref.py.

Kernel forms, each inside poisoned surroundings: the stem, pool + project, the ReLU epilogue of the implicit GEMM (act = 3) at a vector
and a scalar form, the fuse, and the three scribble-tail kernels, which are exact.  The whole detector on the "bounded" checkpoint
(hed_ref.make_state_dict: the one the derived bound says something about) at 64 x 64 (N = 1) and 64 x 128 (N = 3 in groups of 2): the
logit within hed_ref's running bound, the uint8 map inside the interval that bound allows, the scribble output equal to the restated tail
of the detector's own soft map.  On He-initialised checkpoints: a frame's bytes do not depend on its batch or its group, the range guard
raises at scale 1 and runs clean at a small scale.  Every bound is derived (hed_ref's docstring, helpers.igemm_bound); figures are printed
before they are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import helpers
import hed_ref as R
import igemm_forms as IF
from helpers import Guarded, assert_igemm_close

pytestmark = pytest.mark.gpu
U8, F16, F32 = torch.uint8, torch.float16, torch.float32
U8_POISON = 0xA5


@pytest.fixture(scope="module")
def lib(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.ctrl_last_error().decode()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _guard(shape, dtype, dev, data=None, before=96, after=160):
    """a contiguous tensor of `shape` inside a flat allocation; an output's surroundings hold a fixed pattern that must come back, an
    input's hold NaN (uint8: 255) and must not be written either"""
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


# ---------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("N,H,W,scale", [(2, 64, 64, 1.0), (1, 64, 192, 0.25)])
def test_stem(lib, ops, gpu, N, H, W, scale):
    sd = R.make_state_dict(21, "he")
    w, b, norm = sd["block1.convs.0.weight"], sd["block1.convs.0.bias"], sd["norm"].reshape(3)
    frames = R.make_frames(7, N, H, W)
    frames[0, 0, 0] = 255
    frames[0, -1, -1] = 0                                  # the corners: where a wrong padding (0 instead of 0 - norm, or the reverse) shows
    src = _guard((N, H, W, 3), U8, gpu, frames)
    out = _guard((N, H, W, 64), F16, gpu)
    wp = ops.pack_conv_w_direct(w.to(gpu))
    bs = (b * scale).to(gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    nh = (C.c_float * 3)(*[float(v) for v in norm])
    _ok(lib, lib.ctrl_op_hed_stem(_ptr(src.t), N, H, W, _ptr(wp), _ptr(bs), nh, scale, _ptr(out.t), _ptr(flag), _stream()))
    torch.cuda.synchronize()
    x = (frames.permute(0, 3, 1, 2).double() - norm.double().reshape(1, 3, 1, 1)) * scale
    pre = TF.conv2d(x, w.double(), b.double() * scale, padding=1)
    mag = TF.conv2d(x.abs(), w.double().abs(), (b.double() * scale).abs(), padding=1)
    ref = pre.clamp_min(0).permute(0, 2, 3, 1)
    # 27 taps + the subtraction's rounding of every input (the scale is a power of two): K + 1 roundings per term
    assert_igemm_close(out.t, ref, mag.permute(0, 2, 3, 1), 28, 1.0, "hed stem %dx%dx%d s=%g" % (N, H, W, scale))
    assert int(flag[0]) == 0
    src.assert_untouched("stem src")
    out.assert_untouched("stem out")


def test_stem_raises_the_range_flag(lib, ops, gpu):
    sd = R.make_state_dict(21, "he", act_gain=2.0 ** 17)
    frames = R.make_frames(7, 1, 64, 64).to(gpu)
    out = torch.empty((1, 64, 64, 64), dtype=F16, device=gpu)
    flag = torch.zeros(64, dtype=torch.int32, device=gpu)
    nh = (C.c_float * 3)(*[float(v) for v in sd["norm"].reshape(3)])
    _ok(lib, lib.ctrl_op_hed_stem(_ptr(frames), 1, 64, 64, _ptr(ops.pack_conv_w_direct(sd["block1.convs.0.weight"].to(gpu))),
                                  _ptr(sd["block1.convs.0.bias"].to(gpu)), nh, 1.0, _ptr(out), _ptr(flag), _stream()))
    torch.cuda.synchronize()
    assert int(flag[0]) == 1 and bool(torch.isinf(out).any())


# ---------------------------------------------------------------------------------------------------------------- pool + project
@pytest.mark.parametrize("Cc,N,H,W,pool,inv", [(64, 3, 4, 4, True, 1.0), (64, 2, 8, 24, False, 4.0), (512, 3, 4, 4, False, 1.0),
                                               (512, 2, 8, 24, True, 16.0), (128, 1, 8, 24, True, 1.0), (256, 1, 4, 4, True, 2.0)])
def test_pool_proj(lib, gpu, Cc, N, H, W, pool, inv):
    g = torch.Generator().manual_seed(Cc + H)
    h = (torch.randn((N, H, W, Cc), generator=g) * 3).half()
    wp = torch.randn(Cc, generator=g) / Cc ** 0.5
    bp = torch.randn(1, generator=g)
    hd = _guard((N, H, W, Cc), F16, gpu, h)
    p = _guard((N, H, W), F32, gpu)
    pooled = _guard((N, H // 2, W // 2, Cc), F16, gpu) if pool else None
    wd, bd = _guard((Cc,), F32, gpu, wp, before=64, after=64), _guard((1,), F32, gpu, bp, before=64, after=64)
    _ok(lib, lib.ctrl_op_hed_pool_proj(_ptr(hd.t), N, H, W, Cc, _ptr(wd.t), _ptr(bd.t), inv, _ptr(pooled.t if pool else None), _ptr(p.t),
                                       _stream()))
    torch.cuda.synchronize()
    ref = (h.double() * wp.double()).sum(-1) * inv + bp.double()
    mag = (h.double().abs() * wp.double().abs()).sum(-1) * inv + bp.double().abs()
    assert_igemm_close(p.t, ref, mag, Cc, 1.0, "hed pool_proj C%d %dx%dx%d" % (Cc, N, H, W))
    if pool:
        want = TF.max_pool2d(h.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).half()
        assert torch.equal(pooled.t.cpu(), want), "%d pooled values differ" % int((pooled.t.cpu() != want).sum())
        pooled.assert_untouched("pooled")
    for gd in (hd, p, wd, bd):
        gd.assert_untouched("pool_proj")


# ---------------------------------------------------------------------------------------------------------------- ReLU epilogue
@pytest.mark.parametrize("name,nout", [("vector epilogue", 80), ("scalar epilogue", 72)])
def test_igemm_relu_epilogue(ops, gpu, name, nout):
    """act = 3 through ctrl_op_igemm: the element-wise fp64 bound of tests/test_gpu_igemm_forms.py (ReLU is 1-Lipschitz), and the clamp
    exact: no negative output, zero wherever the pre-activation lies below -bound"""
    c = IF.C("hed relu " + name, mode=IF.CONV, n=2, H=7, W=9, Cin=64, Nout=nout, out=IF.F16)
    P = IF.make_problem(ops, gpu, c, seed=3)
    with ops.Profiler() as prof:
        ops.igemm(act=3, **P.kw)
    torch.cuda.synchronize()
    print("FORM %s ran %s" % (c.name, " + ".join(rec[1] or rec[0] for rec in prof.launches)))
    out = P.O.view.detach().cpu()
    assert_igemm_close(out, P.ref.clamp_min(0), P.mag, P.Ktot, 1.0, c.name)
    bound = helpers.igemm_bound(P.ref, P.mag, P.Ktot, 1.0, F16)
    assert not bool((out < 0).any()), "%d negative outputs" % int((out < 0).sum())
    neg = P.ref < -bound
    assert int(neg.sum()) > out.numel() // 4 and bool((out[neg] == 0).all()), "%d outputs below -bound are not zero" % int((out[neg] != 0).sum())
    pos = P.ref > bound
    assert bool((out[pos] > 0).all())
    for gd in (P.A, P.Wg, P.Bg, P.Rv, P.O):
        gd.assert_untouched(c.name)


# ---------------------------------------------------------------------------------------------------------------- fuse
@pytest.mark.parametrize("H,W,ch", [(64, 64, 1), (64, 64, 3), (64, 128, 1), (64, 128, 3)])
def test_fuse(lib, gpu, H, W, ch):
    N = 2
    g = torch.Generator().manual_seed(H + W + ch)
    maps = [torch.randn((N, H >> k, W >> k), generator=g) * 2 for k in range(5)]
    md = [_guard(m.shape, F32, gpu, m, before=64, after=64) for m in maps]
    out = _guard((N, H, W) if ch == 1 else (N, H, W, 3), U8, gpu, before=96, after=96)
    lg = _guard((N, H, W), F32, gpu)
    arr = (C.c_void_p * 5)(*[m.t.data_ptr() for m in md])
    _ok(lib, lib.ctrl_op_hed_fuse(arr, N, H, W, ch, _ptr(out.t), _ptr(lg.t), _stream()))
    torch.cuda.synchronize()
    got, gl = out.t.cpu().numpy(), lg.t.cpu().numpy()
    fails = 0
    for n in range(N):
        ref = sum(R.resize_linear(m[n].double().numpy(), H, W) for m in maps) / 5
        mag = sum(R.resize_linear(m[n].double().abs().numpy(), H, W) for m in maps) / 5
        bound = 16 * 2.0 ** -24 * mag
        nl, nu = R.logit_failures(gl[n], ref, bound), R.u8_failures(got[n] if ch == 1 else got[n][..., 0], ref, bound)
        want_u8, _ = R.fuse([m[n].numpy() for m in maps], H, W)
        diff = int((want_u8 != (got[n] if ch == 1 else got[n][..., 0])).sum())
        print("HED-FUSE %dx%d ch%d frame %d: worst logit err/bound %.3f, bytes outside the interval %d, bytes unlike numpy's %d" % (
            H, W, ch, n, float((np.abs(gl[n] - ref) / bound).max()), nu, diff))
        fails += nl + nu
        if ch == 3:
            assert np.array_equal(got[n][..., 0], got[n][..., 1]) and np.array_equal(got[n][..., 0], got[n][..., 2])
    assert fails == 0
    for gd in md + [out, lg]:
        gd.assert_untouched("fuse")


# ---------------------------------------------------------------------------------------------------------------- the scribble tail
@pytest.mark.parametrize("H,W", [(64, 64), (64, 96)])
def test_tail_stages_are_exact(lib, gpu, H, W):
    maps = R.tail_maps(H, W)
    names = list(maps)
    stack = np.stack([maps[k] for k in names])
    N = len(names)
    src = _guard((N, H, W), U8, gpu, stack)
    # blur to fp32
    bl = _guard((N, H, W), F32, gpu)
    _ok(lib, lib.ctrl_op_hed_blur_f32(_ptr(src.t), N, H, W, _ptr(bl.t), _stream()))
    torch.cuda.synchronize()
    taps = R.gaussian_taps(25)
    want_bl = np.stack([R.blur(maps[k].astype(np.float32), taps) for k in names])
    d = R.exact_failures(bl.t.cpu().numpy(), want_bl)
    print("PARITY hed blur_f32 %dx%d: %d of %d values differ" % (H, W, d, want_bl.size))
    assert d == 0
    # nms: on the raw maps as floats (one-pixel lines, plateaus: the ties) and on the blurred ones
    xin = np.concatenate([stack.astype(np.float32), want_bl])
    xd = _guard(xin.shape, F32, gpu, xin)
    z = _guard(xin.shape, U8, gpu)
    _ok(lib, lib.ctrl_op_hed_nms(_ptr(xd.t), 2 * N, H, W, _ptr(z.t), _stream()))
    torch.cuda.synchronize()
    want_z = np.stack([R.nms_keep(x) for x in xin])
    d = R.exact_failures(z.t.cpu().numpy(), want_z)
    print("PARITY hed nms %dx%d: %d of %d bytes differ; %d kept" % (H, W, d, want_z.size, int((want_z > 0).sum())))
    assert d == 0 and (want_z[:N] > 0).any() and (want_z[N:] > 0).any()
    # blur on uint8 + binarise: on the thinned maps and on the raw ones, 1 and 3 channels
    uin = np.concatenate([want_z, stack])
    ud = _guard(uin.shape, U8, gpu, uin)
    want_o = np.stack([R.blur_u8_bin(u) for u in uin])
    for ch in (1, 3):
        o = _guard(uin.shape if ch == 1 else uin.shape + (3,), U8, gpu)
        _ok(lib, lib.ctrl_op_hed_blur_u8_bin(_ptr(ud.t), uin.shape[0], H, W, ch, _ptr(o.t), _stream()))
        torch.cuda.synchronize()
        got = o.t.cpu().numpy()
        d = R.exact_failures(got if ch == 1 else np.ascontiguousarray(got[..., 1]), want_o)
        print("PARITY hed blur_u8_bin %dx%d ch%d: %d of %d bytes differ; %d set" % (H, W, ch, d, want_o.size, int((want_o > 0).sum())))
        assert d == 0 and (want_o > 0).any()
        if ch == 3:
            assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        o.assert_untouched("blur_u8_bin out")
    for gd in (src, bl, xd, z, ud):
        gd.assert_untouched("tail")


# ---------------------------------------------------------------------------------------------------------------- the whole detector
@pytest.fixture(scope="module")
def bounded(gpu):
    """the bounded checkpoint, its frames and the fp64 logits + bounds, computed once"""
    sd = R.make_state_dict(3, "bounded")
    cases = {}
    for key, (N, H, W) in {"one": (1, 64, 64), "three": (3, 64, 128), "tall": (2, 128, 64), "taller": (1, 192, 64)}.items():
        frames = R.make_frames(5, N, H, W)
        logit, bound = R.logits_and_bound(sd, frames)
        cases[key] = (frames, logit.numpy(), bound.numpy())
    return sd, cases


def _check_detector(det, frames, logit, bound, fpg, what):
    soft, lg = det.run(frames.to(det.device), channels=1, frames_per_group=fpg, return_logits=True)
    soft, lg = soft.cpu().numpy(), lg.cpu().numpy()
    nl, nu = R.logit_failures(lg, logit, bound), R.u8_failures(soft, logit, bound)
    lo, hi = R.u8_interval(logit, bound)
    print("HED-DETECTOR %s: worst logit err/bound %.3f (bound max %.4f, logit std %.3f); %d logits, %d bytes outside; widest interval %d" % (
        what, float((np.abs(lg - logit) / bound).max()), bound.max(), logit.std(), nl, nu, int((hi - lo).max())))
    assert nl == 0 and nu == 0
    scr = det.run(frames.to(det.device), scribble=True, channels=3, frames_per_group=fpg).cpu().numpy()
    for n in range(frames.shape[0]):
        want = R.scribble_tail(soft[n])
        d = R.exact_failures(np.ascontiguousarray(scr[n][..., 0]), want)
        print("PARITY hed scribble %s frame %d: %d of %d bytes differ; %d set" % (what, n, d, want.size, int((want > 0).sum())))
        assert d == 0
        assert np.array_equal(scr[n][..., 0], scr[n][..., 1]) and np.array_equal(scr[n][..., 0], scr[n][..., 2])
    return soft


def test_detector_within_the_derived_bound(gpu, bounded):
    import ctrl_adapter_amd as P
    sd, cases = bounded
    det = P.HEDdetector.from_state_dict(sd, device=gpu)
    soft = _check_detector(det, *cases["one"], None, "64x64 N=1")
    assert len(np.unique(soft)) > 20                       # the map is not flat: the interval check says something
    _check_detector(det, *cases["three"], 2, "64x128 N=3 in groups of 2")


def test_tall_frames_within_the_derived_bound(gpu, bounded):
    """two and three tile rows of the blur, H > W in the fuse, one frame per group: the same derived bound"""
    import ctrl_adapter_amd as P
    sd, cases = bounded
    det = P.HEDdetector.from_state_dict(sd, device=gpu)
    soft = _check_detector(det, *cases["tall"], 1, "128x64 N=2 in groups of 1")
    assert len(np.unique(soft)) > 20
    _check_detector(det, *cases["taller"], 1, "192x64 N=1 in groups of 1")


def test_scale_lever_stays_within_the_bound(gpu, bounded):
    import ctrl_adapter_amd as P
    sd, cases = bounded
    frames, logit, _ = cases["one"]
    _, bound = R.logits_and_bound(sd, frames, trunk_scale=1.0 / 16)
    det = P.HEDdetector.from_state_dict(sd, device=gpu, trunk_scale=1.0 / 16)
    _check_detector(det, frames, logit, bound.numpy(), None, "64x64 N=1 trunk_scale 1/16")


def test_frames_do_not_depend_on_batch_or_group(gpu):
    import ctrl_adapter_amd as P
    det = P.HEDdetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    frames = R.make_frames(9, 3, 64, 128).to(gpu)
    for scribble in (False, True):
        if scribble:
            whole, wl = det.run(frames, scribble=True), None
        else:
            whole, wl = det.run(frames, return_logits=True)
            assert float(wl.std()) > 0.3, "the logits do not spread over the sigmoid: %.3f" % float(wl.std())
        for n in range(3):
            if scribble:
                alone, al = det.run(frames[n:n + 1], scribble=True), None
            else:
                alone, al = det.run(frames[n:n + 1], return_logits=True)
                assert torch.equal(al[0], wl[n]), "frame %d: %d logits differ between N = 1 and N = 3" % (n, int((al[0] != wl[n]).sum()))
            assert torch.equal(alone[0], whole[n]), "frame %d: %d bytes differ between N = 1 and N = 3" % (n, int((alone[0] != whole[n]).sum()))
        for fpg in (1, 2):
            again = det.run(frames, scribble=scribble, frames_per_group=fpg)
            assert torch.equal(again, whole), "frames_per_group=%d: %d bytes differ" % (fpg, int((again != whole).sum()))
        if not scribble:
            assert torch.equal(det.run(frames, return_logits=True, frames_per_group=2)[1], wl)
    assert det.workspace_bytes(3, 64, 128, frames_per_group=1) < det.workspace_bytes(3, 64, 128, frames_per_group=2) \
        <= det.workspace_bytes(3, 64, 128)


def test_tall_frames_do_not_depend_on_batch_or_group(gpu):
    """128 x 64: two tile rows of the blur per frame, H > W in the fuse"""
    import ctrl_adapter_amd as P
    det = P.HEDdetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    frames = R.make_frames(11, 3, 128, 64).to(gpu)
    for scribble in (False, True):
        whole = det.run(frames, scribble=scribble)
        for n in range(3):
            alone = det.run(frames[n:n + 1], scribble=scribble)
            assert torch.equal(alone[0], whole[n]), "frame %d: %d bytes differ between N = 1 and N = 3" % (n, int((alone[0] != whole[n]).sum()))
        for fpg in (1, 2):
            again = det.run(frames, scribble=scribble, frames_per_group=fpg)
            assert torch.equal(again, whole), "frames_per_group=%d: %d bytes differ" % (fpg, int((again != whole).sum()))
    wl = det.run(frames, return_logits=True)[1]
    assert float(wl.std()) > 0.3 and torch.equal(det.run(frames, return_logits=True, frames_per_group=1)[1], wl)
    assert torch.equal(det.run(frames[2:3], return_logits=True)[1][0], wl[2])


def test_range_guard(gpu):
    """a checkpoint whose block 1 leaves the fp16 range (finite inputs, finite weights): the forward says so at scale 1 and runs clean
    at a small scale"""
    import ctrl_adapter_amd as P
    sd = R.make_state_dict(31, "he", act_gain=2.0 ** 17)
    frames = R.make_frames(9, 1, 64, 64).to(gpu)
    det = P.HEDdetector.from_state_dict(sd, device=gpu)
    with pytest.raises(RuntimeError, match="fp16 range"):
        det.run(frames)
    small = P.HEDdetector.from_state_dict(sd, device=gpu, trunk_scale=2.0 ** -8)
    out, lg = small.run(frames, return_logits=True)
    assert bool(torch.isfinite(lg).all()) and out.shape == (1, 64, 64, 3)


def test_extract_scribble_feeds_prepare_images(gpu):
    """raw frames -> scribble map -> controlnet_cond without leaving the device: prepare_images takes extract_scribble's slices as
    they are (uint8 [H, W, 3] on the GPU)"""
    import ctrl_adapter_amd as P
    from oracle import image_prep as O
    from PIL import Image
    det = P.HEDdetector.from_state_dict(R.make_state_dict(31, "he"), device=gpu)
    frames = R.make_frames(9, 2, 64, 64).numpy()
    cond = P.extract_scribble([Image.fromarray(frames[0]), frames[1]], det)
    assert cond.dtype == U8 and cond.shape == (2, 64, 64, 3) and cond.is_cuda and cond.is_contiguous()
    assert set(np.unique(cond.cpu().numpy())) <= {0, 255}
    soft = P.extract_softedge(list(frames), det)
    assert soft.dtype == U8 and soft.shape == (2, 64, 64, 3) and len(torch.unique(soft)) > 20
    assert torch.equal(cond, det(list(frames), detect_resolution=64, image_resolution=64, scribble=True, output_type="pt"))
    pil = P.extract_scribble(list(frames), det, as_pil=True)
    assert np.array_equal(np.asarray(pil[1]), cond[1].cpu().numpy())
    got = P.prepare_images(list(cond), 64, 64, 1, 1, gpu, torch.float16, do_classifier_free_guidance=True)
    want = O.prepare_images([c.cpu().numpy() for c in cond], 64, 64, 1, 1, dtype=torch.float16, do_classifier_free_guidance=True)
    assert got.shape == want.shape == (2, 2, 3, 64, 64) and got.dtype == want.dtype
    assert torch.equal(got.cpu(), want), "%d differing elements" % int((got.cpu() != want).sum())
