"""The canny extractor as far as no GPU is needed: the numpy restatement (tests/canny_ref.py) against cv2's own outputs
(tests/golden/canny/), that those goldens can tell every planted error but the tangent constant, the exported names, every refusal of
the C entries (none reaches a device), the thresholds of the Python wrapper and the sizing queries."""
import ctypes
import os

import numpy as np
import pytest

import helpers  # noqa: F401
import canny_ref as R
from canny_forms import PAIRS, load_pair

SYMBOLS = ("ctrl_op_canny_map", "ctrl_op_canny_hysteresis", "ctrl_op_canny_finish", "ctrl_canny", "ctrl_canny_ws_bytes",
           "ctrl_canny_launch_shape")


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_restatement_equals_cv2_on_the_goldens(i):
    img, want = load_pair(i)
    got = R.canny(img, 100, 200)
    print("golden %s: %d mismatching pixels" % (PAIRS[i][0], int((got != want[..., 0]).sum())))
    assert np.array_equal(got, want[..., 0])


@pytest.mark.parametrize("plant", R.PLANTS)
def test_goldens_tell_every_planted_error_but_the_tangent_constant(plant):
    counts = []
    for i in range(len(PAIRS)):
        img, want = load_pair(i)
        counts.append(int((R.canny(img, 100, 200, plant=plant) != want[..., 0]).sum()))
    print("planted %s: mismatches %s" % (plant, counts))
    if plant == "tangent_13572":
        # known, not shown: 13573 is OpenCV's source's constant and no golden pixel depends on its last unit
        assert counts == [0, 0, 0]
    else:
        assert all(c > 0 for c in counts), counts


def test_small_sizes_follow_the_same_rules():
    g = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 7), (5, 1), (2, 2), (3, 3)):
        img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        m = R.candidate_map(img, 0, 0)
        assert m.shape == (h, w) and set(np.unique(m)) <= {0, 1, 2}
    assert not R.canny(np.zeros((1, 1, 3), np.uint8), 0, 0).any()              # m = 0 is not > 0
    assert not R.canny(np.full((4, 5), 200, np.uint8), 0, 0).any()             # a constant image has no gradient under a replicated border


def test_new_symbols_are_exported_and_the_abi_stays_10():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(helpers.ROOT, "include", "ctrl_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header, name
    assert _lib.ABI_VERSION == 11 and lib.ctrl_abi_version() == 11          # (the name dates from ABI 10: a later entry point bumped it)
    assert callable(P.canny) and callable(P.extract_canny)
    names = [lib.ctrl_policy_name(i).decode() for i in range(lib.ctrl_policy_count())]
    assert "CTRL_CANNY_BATCH" in names


def test_every_refusal_returns_nonzero_before_any_device_is_touched():
    """pointers here are host addresses that are never dereferenced: every call must be refused on its arguments alone"""
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)
    ip, ir = ctypes.c_int(0), ctypes.c_int(0)
    P, RB = ctypes.byref(ip), ctypes.byref(ir)
    npi = ctypes.POINTER(ctypes.c_int)()

    def refused(rc, *words):
        assert rc != 0
        msg = lib.ctrl_last_error().decode()
        assert any(w in msg for w in words), msg
        assert " -> " not in msg, msg                                              # an argument check, not a failed HIP call

    big = (46341, 46341)                                                           # N*H*W*3 > 2^31 - 1 already at N = 1
    # map
    refused(lib.ctrl_op_canny_map(null, 1, 8, 8, 3, 100.0, 200.0, p, null), "null")
    refused(lib.ctrl_op_canny_map(p, 1, 8, 8, 3, 100.0, 200.0, null, null), "null")
    for c in (0, 2, 4):
        refused(lib.ctrl_op_canny_map(p, 1, 8, 8, c, 100.0, 200.0, p, null), "C must be")
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        refused(lib.ctrl_op_canny_map(p, n, h, w, 3, 100.0, 200.0, p, null), "at least 1")
        refused(lib.ctrl_op_canny_hysteresis(p, n, h, w, p, 4096, P, RB, null), "at least 1")
        refused(lib.ctrl_op_canny_finish(p, n, h, w, 3, p, null), "at least 1")
        refused(lib.ctrl_canny(p, n, h, w, 3, 100.0, 200.0, 3, p, p, 4096, P, RB, null), "at least 1")
        assert lib.ctrl_canny_ws_bytes(n, h, w) == 0
    refused(lib.ctrl_op_canny_map(p, 1, big[0], big[1], 3, 100.0, 200.0, p, null), "2^31")
    refused(lib.ctrl_op_canny_map(p, 1, 8, 8, 3, float("nan"), 200.0, p, null), "NaN")
    # hysteresis
    refused(lib.ctrl_op_canny_hysteresis(null, 1, 8, 8, p, 4096, P, RB, null), "null")
    refused(lib.ctrl_op_canny_hysteresis(p, 1, 8, 8, null, 4096, P, RB, null), "null")
    refused(lib.ctrl_op_canny_hysteresis(p, 1, 8, 8, p, 4096, npi, RB, null), "null")
    refused(lib.ctrl_op_canny_hysteresis(p, 1, 8, 8, p, 4096, P, npi, null), "null")
    refused(lib.ctrl_op_canny_hysteresis(p, 1, 8, 8, p, 16, P, RB, null), "workspace")
    refused(lib.ctrl_op_canny_hysteresis(p, 3, 32768, 32768, p, 4096, P, RB, null), "2^31")
    # finish
    refused(lib.ctrl_op_canny_finish(null, 1, 8, 8, 3, p, null), "null")
    refused(lib.ctrl_op_canny_finish(p, 1, 8, 8, 3, null, null), "null")
    for oc in (0, 2, 4):
        refused(lib.ctrl_op_canny_finish(p, 1, 8, 8, oc, p, null), "out_channels")
        refused(lib.ctrl_canny(p, 1, 8, 8, 3, 100.0, 200.0, oc, p, p, 4096, P, RB, null), "out_channels")
    refused(lib.ctrl_op_canny_finish(p, 1, big[0], big[1], 3, p, null), "2^31")
    # the three together
    for args in ((null, p, p), (p, null, p), (p, p, null)):
        refused(lib.ctrl_canny(args[0], 1, 8, 8, 3, 100.0, 200.0, 3, args[1], args[2], 4096, P, RB, null), "null")
    refused(lib.ctrl_canny(p, 1, 8, 8, 3, 100.0, 200.0, 3, p, p, 4096, npi, RB, null), "null")
    for c in (0, 2):
        refused(lib.ctrl_canny(p, 1, 8, 8, c, 100.0, 200.0, 3, p, p, 4096, P, RB, null), "C must be")
    refused(lib.ctrl_canny(p, 1, big[0], big[1], 3, 100.0, 200.0, 1, p, p, 4096, P, RB, null), "2^31")
    refused(lib.ctrl_canny(p, 1, 64, 64, 3, 100.0, 200.0, 3, p, p, 256, P, RB, null), "workspace")
    # launch shape
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    refused(lib.ctrl_canny_launch_shape(8, 8, npi, ctypes.byref(tw)), "null")
    refused(lib.ctrl_canny_launch_shape(0, 8, ctypes.byref(th), ctypes.byref(tw)), "at least 1")
    assert lib.ctrl_canny_ws_bytes(1, big[0], big[1]) == 0


def test_launch_shape_and_workspace_size_are_sane():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    for h, w in ((1, 1), (512, 512), (1024, 1024), (33, 65)):
        assert lib.ctrl_canny_launch_shape(h, w, ctypes.byref(th), ctypes.byref(tw)) == 0
        assert 8 <= th.value <= 256 and 8 <= tw.value <= 256 and tw.value % 4 == 0
    for n, h, w in ((1, 1, 1), (16, 512, 512), (1, 1024, 1024), (3, 33, 65)):
        b = lib.ctrl_canny_ws_bytes(n, h, w)
        assert n * h * w + 64 <= b <= n * h * w + 4096 and b % 16 == 0          # the map, a flag block, padding
    assert lib.ctrl_canny_ws_bytes(2, 64, 64) > lib.ctrl_canny_ws_bytes(1, 64, 64)


def test_wrapper_swaps_and_floors_the_thresholds_and_checks_its_inputs():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.canny import thresholds
    assert thresholds(100, 200) == (100, 200) and thresholds(200, 100) == (100, 200)
    assert thresholds(99.9, 200.5) == (99, 200) and thresholds(200.5, 99.9) == (99, 200)
    assert thresholds(-0.5, 0) == (-1, 0) and thresholds(0, 0) == (0, 0)
    assert thresholds(*thresholds(150.7, 20.2)) == thresholds(150.7, 20.2) == R.thresholds(150.7, 20.2)
    with pytest.raises(ValueError, match="NaN"):
        thresholds(float("nan"), 1)
    from PIL import Image
    rgb = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="mode"):
        P.canny([Image.fromarray(rgb).convert("RGBA")], device="cpu")
    with pytest.raises(ValueError, match="one size"):
        P.canny([rgb, np.zeros((8, 9, 3), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        P.canny([rgb.astype(np.float32)], device="cpu")
    with pytest.raises(ValueError, match="channels"):
        P.canny([rgb], channels=2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # a missing GPU is an error, never a host computation
        P.canny([rgb], device="cpu")
