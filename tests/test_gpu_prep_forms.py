"""The two image-preparation kernels (csrc/imageprep.hip) through ctrl_prepare_images on the table of tests/annot_forms.py: one axis
resampled while the other is not, both, neither, a 1537-tap weight row along each axis, one-pixel sources, work-item counts that leave a
ragged last workgroup and that fill it exactly, F, the batch repeat, the CFG copy and the output type varied across the table.  The weight
tables are those of ctrl_adapter_amd.image_prep._coeffs; the source, both int32 tables of either axis, the scratch image (exactly
F x Hin x W x 3 bytes) and the output lie inside poisoned allocations that must come back untouched.  Bit for bit: the output against
oracle.image_prep.prepare_images, the scratch image against the oracle's horizontal pass.  tests/test_annot_check_host.py pins the oracle to
Pillow at every size of the table and proves that the comparison rejects the planted errors."""
import numpy as np
import pytest
import torch

import annot_forms as A
import helpers
from helpers import Guarded

pytestmark = pytest.mark.gpu
U8, I32 = torch.uint8, torch.int32


@pytest.fixture(scope="module")
def L(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    return _lib


def _guard(shape, dtype, dev, data=None, fill=None, before=96, after=160):
    """a contiguous tensor of `shape` inside a flat allocation: an output between a fixed pattern, an input between `fill`; neither may
    be written outside the tensor (an input: anywhere)"""
    n = int(np.prod(shape))
    if fill is None:
        fill = A.U8_POISON if dtype == U8 else helpers._POISON[dtype]
    g = Guarded((before + n + after,), (slice(before, before + n),), dtype, dev, fill)
    if data is not None:
        g.view.copy_(torch.as_tensor(np.ascontiguousarray(data)).reshape(-1).to(dtype))
        g.is_input = True
    g._snap = helpers._bits(g.buf).clone()
    g.t = g.view.view(*shape)
    return g


def _tables(ks, bounds, kk, gpu):
    """the int32 tables of one axis inside their guards: a bounds entry read from outside names no source pixel at all (first 0, count
    0), a weight read from outside is 1.0 in fixed point -- either shows in the bytes and neither leaves the source"""
    if bounds is None:
        return None, None
    return _guard(bounds.shape, I32, gpu, bounds, fill=0), _guard(kk.shape, I32, gpu, kk, fill=1 << A.PRECISION_BITS)


@pytest.mark.parametrize("kind", list(A.PREP_SIZES))
def test_prepare_images_forms(L, gpu, kind):
    lib = L.lib()
    differ = {"scratch": [0, 0], "out": [0, 0]}          # differing, compared
    for c in (c for c in A.PREP if c.kind == kind):
        hks, hb, hk, vks, vb, vk = A.prep_tables(c)
        src = _guard((c.F, c.Hin, c.Win, 3), U8, gpu, np.stack(A.prep_frames(c.Hin, c.Win, c.F)), fill=255)
        hbg, hkg = _tables(hks, hb, hk, gpu)
        vbg, vkg = _tables(vks, vb, vk, gpu)
        tmp = _guard((c.F, c.Hin, c.W, 3), U8, gpu) if hb is not None else None
        out = _guard((c.cfg, c.rep * c.F, 3, c.H, c.W), c.dt, gpu)
        t = lambda g: L.ptr(g.t if g is not None else None)
        with torch.cuda.device(gpu):
            L.check(lib.ctrl_prepare_images(t(src), c.F, c.Hin, c.Win, t(hbg), t(hkg), hks, t(vbg), t(vkg), vks, t(tmp), t(out), L.dtype_code(c.dt),
                                            c.W, c.H, c.rep, c.cfg, L.cur_stream()))
        torch.cuda.synchronize()
        mid, _ = A.prep_resized(c.Hin, c.Win, c.H, c.W, c.F)
        if tmp is not None:
            d = int((tmp.t.cpu().numpy() != mid).sum())
            differ["scratch"][0] += d
            differ["scratch"][1] += mid.size
            assert d == 0, "%s: %d of %d bytes of the scratch image differ" % (c.id, d, mid.size)
        want = A.prep_expected(c)
        d = A.prep_differs(out.t.cpu(), want)
        differ["out"][0] += d
        differ["out"][1] += want.numel()
        assert d == 0, "%s: %d of %d elements differ" % (c.id, d, want.numel())
        for g in (src, hbg, hkg, vbg, vkg, tmp, out):
            if g is not None:
                g.assert_untouched(c.id)
    print("PARITY prepare_images %s: resample_h %d of %d bytes differ, resample_v_store %d of %d elements differ" % (
        kind, differ["scratch"][0], differ["scratch"][1], differ["out"][0], differ["out"][1]))
    assert differ["out"][1] > 0 and (differ["scratch"][1] > 0) == (kind not in ("v", "neither"))
