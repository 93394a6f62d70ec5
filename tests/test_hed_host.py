"""No GPU needed.  The HED restatement (tests/hed_ref.py) and the checks tests/test_gpu_hed.py applies to the library: every planted
error must be caught by the very check the GPU side uses; the restatement is pinned to controlnet_aux and cv2 wherever those packages
exist (neither is installed here: the two pins run as skips and README / DESIGN say "not pinned"); the ABI and the Python entry's refusals."""
import numpy as np
import pytest
import torch

import hed_ref as R
from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)

H, W = 64, 64


@pytest.fixture(scope="module")
def bounded_case():
    sd = R.make_state_dict(3, "bounded")
    frames = R.make_frames(5, 1, H, W)
    logit, bound = R.logits_and_bound(sd, frames)
    return sd, frames, logit.numpy(), bound.numpy()


def test_bound_is_useful_and_the_logits_spread(bounded_case):
    """the derived bound of the bounded checkpoint is far below the spread of the logits, and the logits cross the sigmoid's middle:
    a check against it can fail"""
    _, _, logit, bound = bounded_case
    print("HED-REF logit min %.3f max %.3f std %.3f | bound max %.4f median %.4f" % (logit.min(), logit.max(), logit.std(), bound.max(),
                                                                                      np.median(bound)))
    assert logit.std() > 0.3 and logit.min() < 0 < logit.max()
    assert bound.max() < 0.25 * logit.std()
    lo, hi = R.u8_interval(logit, bound)
    assert (hi - lo).max() <= 16 and len(np.unique(lo)) > 20


def test_restatement_passes_its_own_checks(bounded_case):
    sd, frames, logit, bound = bounded_case
    m = R.ControlNetHEDRef()
    m.load_state_dict(sd)
    with torch.no_grad():
        maps = m(frames.permute(0, 3, 1, 2).float())
    u8, mean = R.fuse([p[0, 0].numpy() for p in maps], H, W)
    assert R.logit_failures(mean, logit, bound) == 0
    assert R.u8_failures(u8, logit, bound) == 0


@pytest.mark.parametrize("planted", [dict(pool_blocks=(0, 1, 2, 3)), dict(pool_blocks=(1, 2, 3)), dict(no_relu_last=0), dict(no_relu_last=2),
                                     dict(no_relu_last=4), dict(align_corners=True)],
                         ids=["pool-one-block-early", "pool-missing-before-block5", "no-relu-block1", "no-relu-block3", "no-relu-block5",
                              "align-corners"])
def test_planted_model_errors_are_caught(bounded_case, planted):
    sd, frames, logit, bound = bounded_case
    if planted.get("pool_blocks") == (0, 1, 2, 3):
        big = R.make_frames(5, 1, 2 * H, 2 * W)          # the early pool halves every map: the same output size from a frame twice as large
        bad, _ = R.logits_and_bound(sd, big, want_bound=False, **planted)
        bad = bad[:, ::2, ::2]
    elif planted.get("pool_blocks") == (1, 2, 3):
        # block 5 without its pool: its map arrives at stride 8 -- resized from there
        bad, _ = R.logits_and_bound(sd, frames, want_bound=False, **planted)
    else:
        bad, _ = R.logits_and_bound(sd, frames, want_bound=False, **planted)
    bad = bad.numpy()
    nl = R.logit_failures(bad, logit, bound)
    u8 = (255.0 / (1.0 + np.exp(-bad))).clip(0, 255).astype(np.uint8)
    nu = R.u8_failures(u8, logit, bound)
    print("HED-PLANTED %s: %d logits, %d bytes of %d outside" % (planted, nl, nu, logit.size))
    assert nl > logit.size // 20 and nu > logit.size // 50


@pytest.mark.parametrize("planted", [dict(border="reflect"), dict(directions=3), dict(swap_ksize=True)],
                         ids=["reflect-not-101", "nms-without-a-diagonal", "ksize-25-19-swapped"])
def test_planted_tail_errors_are_caught(planted):
    moved = {}
    for shape in ((64, 64), (64, 96)):
        for name, m in R.tail_maps(*shape).items():
            moved[(shape, name)] = R.exact_failures(R.scribble_tail(m, **planted), R.scribble_tail(m))
    print("HED-PLANTED-TAIL %s: %s" % (planted, moved))
    assert sum(1 for v in moved.values() if v) >= 2, moved


def test_tail_maps_exercise_the_tail():
    for name, m in R.tail_maps(64, 96).items():
        z, x = R.nms(m)
        out = R.scribble_tail(m)
        assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 255}
        if name in ("plateaus", "random", "waves"):          # (a blurred one-pixel line stays below the threshold: those maps serve the stage tests)
            assert z.any() and out.any(), name


def test_taps():
    for n, u8 in ((25, False), (19, True)):
        assert R.auto_ksize(3.0, u8) == n
        t = R.gaussian_taps(n)
        assert t.dtype == np.float32 and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(t, t[::-1])


def test_resize_linear_clamps_and_copies():
    e = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(R.resize_linear(e, 3, 4), e)
    up = R.resize_linear(e, 48, 64)
    assert up.dtype == np.float32 and up[0, 0] == e[0, 0] and up[-1, -1] == e[-1, -1] and up[0, 7] == e[0, 0]       # both clamps
    assert abs(up[0, 8] - (e[0, 0] * (1 - 1 / 32) + e[0, 1] / 32)) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- pins
def test_pin_net_and_detector_to_controlnet_aux():
    aux = pytest.importorskip("controlnet_aux")
    from controlnet_aux.hed import ControlNetHED_Apache2
    sd = R.make_state_dict(11, "he")
    net = ControlNetHED_Apache2().float().eval()
    net.load_state_dict(sd)
    mine = R.ControlNetHEDRef().eval()
    mine.load_state_dict(sd)
    frames = R.make_frames(2, 1, 128, 128)
    x = frames.permute(0, 3, 1, 2).float()
    with torch.no_grad():
        a, b = net(x), mine(x)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    det = aux.HEDdetector(net)
    img = frames[0].numpy()
    soft = det(img, detect_resolution=128, image_resolution=128, output_type="np")
    want, _ = R.fuse([p[0, 0].numpy() for p in b], 128, 128)
    assert np.array_equal(np.asarray(soft)[..., 0], want)
    scr = det(img, detect_resolution=128, image_resolution=128, scribble=True, output_type="np")
    assert np.array_equal(np.asarray(scr)[..., 0], R.scribble_tail(want))


def test_pin_tail_and_bilinear_to_cv2():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.RandomState(0)
    for (h, w), (oh, ow) in (((4, 4), (64, 64)), ((4, 8), (64, 128)), ((32, 64), (64, 128)), ((256, 256), (512, 512))):
        e = rng.randn(h, w).astype(np.float32)
        assert np.array_equal(cv2.resize(e, (ow, oh), interpolation=cv2.INTER_LINEAR), R.resize_linear(e, oh, ow))
    for shape in ((64, 64), (64, 96)):
        for name, m in R.tail_maps(*shape).items():
            x = cv2.GaussianBlur(m.astype(np.float32), (0, 0), 3.0)
            assert np.array_equal(x, R.nms(m)[1]), name
            z = R.nms(m)[0]
            got = cv2.GaussianBlur(z, (0, 0), 3.0)
            got[got > 4] = 255
            got[got < 255] = 0
            assert np.array_equal(got, R.blur_u8_bin(z)), name


# ---------------------------------------------------------------------------------------------------------------- ABI and refusals
def test_abi_symbols_present():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_hed_create", "ctrl_hed_forward", "ctrl_hed_destroy", "ctrl_hed_ws_bytes", "ctrl_op_hed_stem", "ctrl_op_hed_pool_proj",
                 "ctrl_op_hed_fuse", "ctrl_op_hed_blur_f32", "ctrl_op_hed_nms", "ctrl_op_hed_blur_u8_bin"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    import ctypes
    assert ctypes.sizeof(_lib.HedConfig) == 16


def test_python_entry_refuses_what_it_cannot_do():
    import ctrl_adapter_amd as P
    assert P.HEDdetector is not None and P.extract_scribble is not None and P.extract_softedge is not None
    from ctrl_adapter_amd import hed
    assert [n for n, _ in hed.hed_state_dict_spec()] == [n for n, _ in R.spec()]
    det = object.__new__(P.HEDdetector)          # no GPU here: the refusals come before anything touches the plan
    det._plan = None
    det.device = torch.device("cpu")
    img = np.zeros((512, 512, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        det(img, safe=True)
    with pytest.raises(ValueError, match="resized"):
        det(np.zeros((480, 512, 3), np.uint8))
    with pytest.raises(ValueError, match="resized"):
        det(img, detect_resolution=384)
    with pytest.raises(ValueError, match="resized"):
        det(np.zeros((512, 768, 3), np.uint8), image_resolution=768)
    with pytest.raises(ValueError, match="one size"):
        det([img, np.zeros((512, 576, 3), np.uint8)])
    with pytest.raises(ValueError):
        det(np.zeros((512, 512, 4), np.uint8))
    with pytest.raises(ValueError):
        det(img, output_type="latent")
    det.device = torch.device("cuda:0")
    assert det.to("cuda") is det and det.to("cuda:0") is det          # the helper's `.to("cuda")` is a no-op on the plan's own GPU
    with pytest.raises(ValueError):
        det.to("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.HEDdetector(R.make_state_dict(1))
    with pytest.raises(TypeError):
        P.extract_scribble([img], detector=None)
