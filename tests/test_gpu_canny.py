"""The canny extractor on the GPU (csrc/canny.hip, ctrl_adapter_amd.canny): the public interface against cv2's own outputs
(tests/golden/canny/), the map kernel against the numpy restatement (tests/canny_ref.py) at every size, threshold pair and input of
tests/canny_forms.py, the hysteresis op on synthetic maps against a flood fill, the finish kernel, batches, repeatability and the
chain into prepare_images.  Every comparison is exact: the number of differing bytes is printed and
must be 0.  Device operands are contiguous tensors placed at every byte phase inside a larger allocation: an input's surroundings
hold 255 (a halo read past the image would raise magnitudes and show), an output's hold a fixed pattern that must come back.
Not here: the refusal of a capturing stream.  A test that opened a capture (torch.cuda.graph) around the refused calls passed, but
with it in the suite's process a later graph replay of the adapter (tests/test_gpu_e2e.py) ended in a segmentation fault, as DESIGN.md
section 7 records for other captures added ahead of that test; the cause is not known, so no capture is opened here."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import canny_forms as F
import canny_ref as R
from helpers import Guarded

pytestmark = pytest.mark.gpu
U8 = torch.uint8
POISON = 0xA5            # neither 0, 1, 2 nor 255


@pytest.fixture(scope="module")
def lib(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def tile(lib):
    th, tw = C.c_int(0), C.c_int(0)
    assert lib.ctrl_canny_launch_shape(512, 512, C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def _guard(shape, before, after, dev, fill, data=None):
    """a contiguous uint8 tensor of `shape` that starts `before` bytes into a flat allocation and ends `after` bytes before its end;
    the rest holds `fill` (helpers.Guarded has no uint8 poison of its own: built from its constructor)"""
    n = int(np.prod(shape))
    g = Guarded((before + n + after,), (slice(before, before + n),), U8, dev, fill)
    if data is not None:
        g.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1))
        g.is_input = True
    g._snap = helpers._bits(g.buf).clone()
    g.t = g.view.view(*shape)
    assert g.t.is_contiguous() and g.t.data_ptr() == g.buf.data_ptr() + before
    return g


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.ctrl_last_error().decode()


def _same(what, got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = int((got != want).sum())
    if bad:
        idx = np.argwhere(got != want)[0]
        raise AssertionError("%s: %d differing bytes; first at %s: got %d, wanted %d" % (what, bad, tuple(idx), got[tuple(idx)], want[tuple(idx)]))
    return 0


def _hysteresis(lib, dev, maps, before=0):
    """maps uint8 [N, H, W] on the host -> (result [N, H, W] on the host, passes, readbacks), through ctrl_op_canny_hysteresis in place"""
    N, H, W = maps.shape
    g = _guard((N, H, W), before, 7, dev, POISON)
    g.t.copy_(torch.from_numpy(maps))
    ws = torch.empty(int(lib.ctrl_canny_ws_bytes(N, H, W)), dtype=U8, device=dev)
    p, r = C.c_int(-1), C.c_int(-1)
    _ok(lib, lib.ctrl_op_canny_hysteresis(g.t.data_ptr(), N, H, W, ws.data_ptr(), ws.numel(), C.byref(p), C.byref(r), _stream()))
    torch.cuda.synchronize()
    g.assert_untouched("hysteresis")
    return g.t.cpu().numpy(), p.value, r.value


# ---- the public interface on the goldens -----------------------------------------------------------------------------------------
def test_canny_and_extract_canny_reproduce_cv2_on_the_goldens(gpu):
    import ctrl_adapter_amd as P
    from PIL import Image
    imgs = [F.load_pair(i)[0] for i in range(len(F.PAIRS))]
    want3 = np.stack([F.load_pair(i)[1] for i in range(len(F.PAIRS))])
    want1 = np.ascontiguousarray(want3[..., 0])
    forms = {"PIL": [Image.fromarray(i) for i in imgs], "numpy": imgs, "device tensors": [torch.from_numpy(i.copy()).to(gpu) for i in imgs],
             "host tensors": [torch.from_numpy(i.copy()) for i in imgs]}
    for name, inp in forms.items():
        got, stats = P.canny(inp, return_stats=True)
        assert got.is_cuda and got.dtype == U8
        print("PARITY canny from %s vs cv2: %d differing bytes of %d; passes %d, readbacks %d" % (
            name, _same("canny from " + name, got, want1), want1.size, stats["passes"], stats["readbacks"]))
        assert stats["passes"] >= 1 and 1 <= stats["readbacks"] <= stats["passes"]
        got3 = P.extract_canny(inp)
        assert got3.is_cuda and got3.dtype == U8
        print("PARITY extract_canny from %s vs cv2: %d differing bytes" % (name, _same("extract_canny from " + name, got3, want3)))
    _same("canny, channels=3", P.canny(imgs, 100, 200, channels=3, device=gpu), want3)
    _same("canny, thresholds swapped", P.canny(imgs[:1], 200, 100), want1[:1])
    # one channel in: mode L through np.array, as the reference would hand it to cv2
    grey = [Image.fromarray(i).convert("L") for i in imgs[:2]]
    _same("canny from mode L", P.canny(grey), np.stack([R.canny(np.array(g)) for g in grey]))
    # as_pil: the PIL images the reference's pipelines expect, and they go back in
    pil = P.extract_canny(forms["PIL"], as_pil=True)
    assert len(pil) == 3 and all(p.mode == "RGB" and p.size == (512, 512) for p in pil)
    _same("extract_canny(as_pil=True)", np.stack([np.array(p) for p in pil]), want3)
    again = P.extract_canny(pil)                        # an edge map's edges: any image is an input
    _same("extract_canny of its own PIL output", again, np.stack([np.stack([R.canny(np.array(p))] * 3, axis=2) for p in pil]))


# ---- the map kernel -----------------------------------------------------------------------------------------------------------
def _map_cases():
    # the tile is only known on the GPU machine: the cases are indices into map_sizes(th, tw), whose length does not depend on it
    return [(i, c) for i in range(len(F.map_sizes(64, 64))) for c in (1, 3)]


@pytest.mark.parametrize("size_index,chans", _map_cases())
def test_map_kernel_equals_the_restatement(lib, gpu, tile, size_index, chans):
    H, W = F.map_sizes(*tile)[size_index]
    inputs = F.map_inputs(H, W, chans, seed=100 * size_index + chans)
    names = sorted(inputs)
    batch = np.stack([inputs[k] for k in names])                     # [N, H, W, C]: every input image of this size in one launch
    N = len(names)
    worst = 0
    for k, (low, high) in enumerate(F.THRESHOLDS):
        want = np.stack([R.candidate_map(batch[n] if chans == 3 else batch[n][..., 0], low, high) for n in range(N)])
        blurred = want[names.index("blurred")]
        if (low, high) == (2040, 3000):
            assert not want.any()                                    # no magnitude exceeds 2040
        elif min(H, W) >= 16 and min(low, high) >= 99:
            # blurred noise straddles both thresholds (a smaller image cannot hold all three classes, and with low = high = 0 nothing is weak)
            assert all((blurred == v).any() for v in (0, 1, 2)), (H, W, chans, low, high)
        src = _guard((N, H, W, chans), k % 4, 3 + k, gpu, 255, batch if chans == 3 else batch[..., 0])
        out = _guard((N, H, W), (3 * k + 1) % 4 if k else 0, 5, gpu, POISON)
        _ok(lib, lib.ctrl_op_canny_map(src.t.data_ptr(), N, H, W, chans, float(low), float(high), out.t.data_ptr(), _stream()))
        torch.cuda.synchronize()
        for n in range(N):
            worst += _same("map %dx%dx%d %s at (%s, %s)" % (H, W, chans, names[n], low, high), out.t[n], want[n])
        src.assert_untouched("map input")
        out.assert_untouched("map output")
    print("PARITY canny map %dx%d C=%d: %d inputs x %d threshold pairs, %d differing bytes" % (H, W, chans, N, len(F.THRESHOLDS), worst))


# ---- the hysteresis op ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hmaps(tile):
    maps = F.hysteresis_maps(*tile)
    return maps, {k: R.hysteresis(v) for k, v in maps.items()}      # the flood fills, computed once


@pytest.mark.parametrize("name", ["serpentine", "diagonal_junctions", "weak_only_components", "all_none", "all_weak", "all_strong", "corners",
                                  "random", "ragged", "ragged_serpentine"])
def test_hysteresis_equals_the_flood_fill(lib, gpu, tile, hmaps, name):
    m, want = hmaps[0][name], hmaps[1][name]
    th, tw = tile
    if not name.startswith("ragged"):
        assert m.shape == (3 * th, 3 * tw)
    else:
        assert m.shape == (2 * th + 1, 2 * tw - 1)
    got, passes, readbacks = _hysteresis(lib, gpu, m[None], before={"ragged": 1, "random": 2, "corners": 3}.get(name, 0))
    print("PARITY canny hysteresis %s %dx%d: %d differing bytes; passes %d, readbacks %d" % (
        name, m.shape[0], m.shape[1], _same("hysteresis " + name, got[0], want), passes, readbacks))
    assert passes >= 1 and 1 <= readbacks <= passes
    if name == "serpentine":
        assert F.crossings(m, th, tw) >= 20 and (want != 1).all() and (want == 2).sum() == (m != 0).sum()
        assert passes >= 2                                           # the multi-pass path ran
    if name == "diagonal_junctions":
        assert (want != 1).all() and m[th - 1, tw - 1] == 1 and m[th, tw] == 1 and m[th - 1, 2 * tw] == 1 and m[th, 2 * tw - 1] == 1
        assert not m[th - 1, tw] and not m[th, tw - 1]              # the corner is crossed by a diagonal step, nothing beside it
    if name in ("weak_only_components", "all_weak"):
        assert (want == 1).sum() == (m == 1).sum() > 0              # nothing to promote: one pass says so
        assert passes == 1
    if name in ("all_none", "all_strong"):
        assert passes == 1 and np.array_equal(want, m)
    # the finish of this map, on one channel and on three, at odd byte phases
    N, (H, W) = 1, m.shape
    src = _guard((N, H, W), 1, 3, gpu, POISON, got)
    for oc, before in ((1, 2), (3, 1), (3, 0), (1, 0)):
        out = _guard((N, H, W) if oc == 1 else (N, H, W, 3), before, 6, gpu, POISON)
        _ok(lib, lib.ctrl_op_canny_finish(src.t.data_ptr(), N, H, W, oc, out.t.data_ptr(), _stream()))
        torch.cuda.synchronize()
        e = np.where(want == 2, 255, 0).astype(np.uint8)[None]
        _same("finish %s on %d channel(s)" % (name, oc), out.t, e if oc == 1 else np.stack([e] * 3, axis=3))
        out.assert_untouched("finish output")
    src.assert_untouched("finish input")


def test_a_batch_equals_its_single_calls_and_does_not_stop_early(lib, gpu, tile, hmaps):
    import ctrl_adapter_amd as P
    maps, fills = hmaps
    # a serpentine beside an empty map, in both orders: the empty image's tiles promote nothing from the first pass on
    for order in (("all_none", "serpentine"), ("serpentine", "all_none"), ("serpentine", "random", "corners")):
        got, passes, readbacks = _hysteresis(lib, gpu, np.stack([maps[k] for k in order]))
        for n, k in enumerate(order):
            _same("hysteresis batch %s[%d]" % (order, n), got[n], fills[k])
        assert passes >= 2
        print("PARITY canny hysteresis batch %s: exact; passes %d, readbacks %d" % ("+".join(order), passes, readbacks))
    # the whole extractor: three images of different content in one call, and each alone
    imgs = [np.ascontiguousarray(F.load_pair(i)[0][100:100 + 2 * tile[0] + 5, 60:60 + 2 * tile[1] - 3]) for i in range(3)]
    together = P.canny(imgs, 100, 200, channels=3, device=gpu)
    for n, img in enumerate(imgs):
        alone = P.canny([img], 100, 200, channels=3, device=gpu)
        assert torch.equal(alone[0], together[n]), "image %d differs between the batch and its own call" % n
        _same("batch image %d vs the restatement" % n, together[n], np.stack([R.canny(img)] * 3, axis=2))
    # the same call twice: identical bytes
    assert torch.equal(together, P.canny(imgs, 100, 200, channels=3, device=gpu))


def test_extracted_conditions_feed_prepare_images(gpu):
    """raw frame -> edge map -> controlnet_cond without leaving the device: prepare_images takes extract_canny's slices as they are"""
    import ctrl_adapter_amd as P
    from oracle import image_prep as O
    imgs = [np.ascontiguousarray(F.load_pair(i)[0][200:296, 150:270]) for i in range(2)]             # 96 x 120
    cond = P.extract_canny(imgs)
    got = P.prepare_images(list(cond), 64, 64, 1, 1, gpu, torch.float16, do_classifier_free_guidance=True)
    want = O.prepare_images([np.stack([R.canny(i)] * 3, axis=2) for i in imgs], 64, 64, 1, 1, dtype=torch.float16,
                            do_classifier_free_guidance=True)
    assert got.shape == want.shape == (2, 2, 3, 64, 64) and got.dtype == want.dtype
    assert torch.equal(got.cpu(), want), "%d differing elements" % int((got.cpu() != want).sum())
    print("PARITY extract_canny -> prepare_images vs the oracle on the restatement: bit-exact")
