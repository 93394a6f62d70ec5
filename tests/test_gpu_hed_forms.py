"""The HED annotator's memory-bound kernels (csrc/hed.hip) at their quad and tile edges, on the tables of tests/annot_forms.py: the stem
with a ragged last workgroup, one quad per row, H < 3 and a tall frame; pool + project with a ragged last workgroup for every C; the
fuse at H > W, with a deepest side map of 1 x 1 and 1 x 3 and a ragged last workgroup; the three scribble-tail kernels on maps with a
second tile row, partial tiles both ways, maps narrower than a tile and W % 4 != 0, and nms down to 1 x 1.  References and bounds are
those of tests/test_gpu_hed.py, unchanged; every input, output and weight lies inside a poisoned allocation that must come back untouched.
tests/test_annot_check_host.py holds the tables' edges and proves that the checks reject the planted errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import annot_forms as A
import hed_ref as R
import helpers
from helpers import Guarded, assert_igemm_close

pytestmark = pytest.mark.gpu
U8, F16, F32 = torch.uint8, torch.float16, torch.float32


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
        fill = A.U8_POISON if dtype == U8 else helpers._POISON[dtype]
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
def test_stem_forms(lib, ops, gpu):
    worst = 0.0
    for N, H, W in A.STEM_SIZES:
        frames, w, b, norm, scale, ref, mag = A.hed_stem_problem(N, H, W)
        src = _guard((N, H, W, 3), U8, gpu, frames)
        out = _guard((N, H, W, 64), F16, gpu)
        wp = _guard((27 * 64,), F32, gpu, ops.pack_conv_w_direct(w.to(gpu)).reshape(-1).cpu())
        bs = _guard((64,), F32, gpu, b * scale)
        flag = torch.zeros(64, dtype=torch.int32, device=gpu)
        nh = (C.c_float * 3)(*[float(v) for v in norm])
        _ok(lib, lib.ctrl_op_hed_stem(_ptr(src.t), N, H, W, _ptr(wp.t), _ptr(bs.t), nh, scale, _ptr(out.t), _ptr(flag), _stream()))
        torch.cuda.synchronize()
        share, _ = assert_igemm_close(out.t, ref, mag, 28, 1.0, "hed stem %dx%dx%d s=%g" % (N, H, W, scale))
        worst = max(worst, share)
        assert int(flag[0]) == 0
        for gd in (src, out, wp, bs):
            gd.assert_untouched("stem %dx%dx%d" % (N, H, W))
    print("PARITY hed stem: worst |err| / bound %.3f over %d sizes" % (worst, len(A.STEM_SIZES)))


# ---------------------------------------------------------------------------------------------------------------- pool + project
@pytest.mark.parametrize("Cc", A.POOL_CS)
def test_pool_proj_forms(lib, gpu, Cc):
    worst, differ = 0.0, 0
    for c in (c for c in A.POOL if c.C == Cc):
        h, wp, bp, ref, mag, want = A.pool_problem(c.id)
        hd = _guard((c.N, c.H, c.W, Cc), F16, gpu, h)
        p = _guard((c.N, c.H, c.W), F32, gpu)
        pooled = _guard((c.N, c.H // 2, c.W // 2, Cc), F16, gpu) if c.pooled else None
        wd, bd = _guard((Cc,), F32, gpu, wp, before=64, after=64), _guard((1,), F32, gpu, bp, before=64, after=64)
        _ok(lib, lib.ctrl_op_hed_pool_proj(_ptr(hd.t), c.N, c.H, c.W, Cc, _ptr(wd.t), _ptr(bd.t), c.inv, _ptr(pooled.t if c.pooled else None),
                                           _ptr(p.t), _stream()))
        torch.cuda.synchronize()
        share, _ = assert_igemm_close(p.t, ref, mag, Cc, 1.0, c.id)
        worst = max(worst, share)
        if c.pooled:
            d = int((pooled.t.cpu() != want).sum())
            differ += d
            assert d == 0, "%s: %d pooled values differ" % (c.id, d)
            pooled.assert_untouched(c.id + " pooled")
        for gd in (hd, p, wd, bd):
            gd.assert_untouched(c.id)
    print("PARITY hed pool_proj<%d>: worst |err| / bound %.3f, %d pooled values differ" % (Cc // 8, worst, differ))


# ---------------------------------------------------------------------------------------------------------------- fuse
@pytest.mark.parametrize("ch", A.FUSE_CHANNELS)
def test_fuse_forms(lib, gpu, ch):
    worst, unlike = 0.0, 0
    for N, H, W in A.FUSE_SIZES:
        maps, ref, bound, want = A.hed_fuse_problem(N, H, W)
        md = [_guard(m.shape, F32, gpu, m, before=64, after=64) for m in maps]
        out = _guard((N, H, W) if ch == 1 else (N, H, W, 3), U8, gpu, before=96, after=96)
        lg = _guard((N, H, W), F32, gpu)
        arr = (C.c_void_p * 5)(*[m.t.data_ptr() for m in md])
        _ok(lib, lib.ctrl_op_hed_fuse(arr, N, H, W, ch, _ptr(out.t), _ptr(lg.t), _stream()))
        torch.cuda.synchronize()
        got = out.t.cpu().numpy()
        first = got if ch == 1 else np.ascontiguousarray(got[..., 0])
        share, nl, nu = A.hed_fuse_check(first, lg.t.cpu().numpy(), ref, bound)
        d = int((first != want).sum())
        print("HED-FUSE %dx%dx%d ch%d: worst logit err/bound %.3f, %d logits and %d bytes outside, %d bytes unlike numpy's" % (N, H, W, ch, share, nl, nu, d))
        worst, unlike = max(worst, share), unlike + d
        assert nl == 0 and nu == 0, (N, H, W)
        if ch == 3:
            assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        for gd in md + [out, lg]:
            gd.assert_untouched("fuse %dx%dx%d" % (N, H, W))
    print("PARITY hed fuse<%d>: worst |err| / bound %.3f, %d bytes unlike numpy's" % (ch, worst, unlike))


# ---------------------------------------------------------------------------------------------------------------- the scribble tail
@pytest.mark.parametrize("N", A.TAIL_NS)
def test_tail_forms_are_exact(lib, gpu, N):
    count = {"blur_f32": [0, 0], "nms": [0, 0], "blur_u8_bin": [0, 0]}          # differing, compared
    for H, W in A.BLUR_SIZES + A.BLUR_U8_ONLY + A.NMS_ONLY:
        ref = A.tail_reference(N, H, W)
        what = "tail N%d %dx%d" % (N, H, W)
        src = _guard((N, H, W), U8, gpu, ref["stack"])
        if "blur" in ref:
            bl = _guard((N, H, W), F32, gpu)
            _ok(lib, lib.ctrl_op_hed_blur_f32(_ptr(src.t), N, H, W, _ptr(bl.t), _stream()))
            torch.cuda.synchronize()
            d = R.exact_failures(bl.t.cpu().numpy(), ref["blur"])
            count["blur_f32"][0] += d
            count["blur_f32"][1] += ref["blur"].size
            assert d == 0, "%s blur_f32: %d of %d values differ" % (what, d, ref["blur"].size)
            bl.assert_untouched(what + " blur_f32")
        xin, want_z = ref["nms_in"], ref["nms"]
        xd = _guard(xin.shape, F32, gpu, xin)
        z = _guard(xin.shape, U8, gpu)
        _ok(lib, lib.ctrl_op_hed_nms(_ptr(xd.t), xin.shape[0], H, W, _ptr(z.t), _stream()))
        torch.cuda.synchronize()
        d = R.exact_failures(z.t.cpu().numpy(), want_z)
        count["nms"][0] += d
        count["nms"][1] += want_z.size
        assert d == 0 and (want_z > 0).any(), "%s nms: %d of %d bytes differ" % (what, d, want_z.size)
        for gd in (src, xd, z):
            gd.assert_untouched(what + " nms")
        if "bin" in ref:
            uin, want_o = ref["bin_in"], ref["bin"]
            ud = _guard(uin.shape, U8, gpu, uin)
            for ch in (1, 3):
                o = _guard(uin.shape if ch == 1 else uin.shape + (3,), U8, gpu)
                _ok(lib, lib.ctrl_op_hed_blur_u8_bin(_ptr(ud.t), uin.shape[0], H, W, ch, _ptr(o.t), _stream()))
                torch.cuda.synchronize()
                got = o.t.cpu().numpy()
                d = R.exact_failures(got if ch == 1 else np.ascontiguousarray(got[..., 1]), want_o)
                count["blur_u8_bin"][0] += d
                count["blur_u8_bin"][1] += want_o.size
                assert d == 0 and (want_o > 0).any(), "%s blur_u8_bin ch%d: %d of %d bytes differ" % (what, ch, d, want_o.size)
                if ch == 3:
                    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
                o.assert_untouched(what + " blur_u8_bin out")
            ud.assert_untouched(what + " blur_u8_bin in")
    for k, (d, n) in count.items():
        print("PARITY hed %s N=%d: %d of %d values differ" % (k, N, d, n))
        assert n > 0
