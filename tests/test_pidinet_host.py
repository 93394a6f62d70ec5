"""No GPU needed.  The PiDiNet restatement (tests/pidinet_ref.py) and the checks tests/test_gpu_pidinet.py applies to the library: the
host-side PDC conversion against the restatement and the restatement's conversion against the on-the-fly formulas; every planted error
must be caught by the very check the GPU side uses; the restatement is pinned to controlnet_aux wherever that package exists (it is not
installed here: the pin runs as a skip and README / DESIGN say "not pinned"); the ABI and the Python entry's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pidinet_forms as PF
import pidinet_ref as R
from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)


def _asym(co, ci, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((co, ci, 3, 3), generator=g) + 0.1 * torch.arange(9.0).reshape(1, 1, 3, 3)).float()


@pytest.mark.parametrize("kind", ["cv", "cd", "ad", "rd"])
def test_convert_pdc(kind):
    """the library's host conversion equals the restatement's (computed in double, rounded once to fp32), and the restatement's kernel
    computes what the on-the-fly formula computes, full and depthwise, within 1e-12 relative in fp64"""
    for co, ci, groups in ((7, 3, 1), (12, 1, 12)):
        w = _asym(co, ci, 5 + co)
        ref = R.convert_pdc(kind, w.double())
        got = PF.lib_convert(kind, w)
        assert got.shape == ref.shape
        err = (got.double() - ref.float().double()).abs()
        assert bool((err <= 1e-12 * ref.abs()).all()), float(err.max())
        x = torch.randn((2, ci * groups, 9, 11), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        a = R.pdc_on_the_fly(kind, x, w.double(), groups)
        b = F.conv2d(x, ref, padding=ref.shape[-1] // 2, groups=groups)
        rel = float((a - b).abs().max() / a.abs().max())
        print("PIDI-CONVERT %s groups %d: converted vs on the fly %.2e" % (kind, groups, rel))
        assert rel < 1e-12
    if kind == "rd":        # the footprint the block kernel reads: sixteen positions, the other nine exactly zero
        z = PF.lib_convert(kind, _asym(4, 1, 2)).reshape(4, 25)
        unused = [i for i in range(25) if i not in R.RD_POS + R.RD_NEG]
        assert bool((z[:, unused] == 0).all()) and bool((z[:, R.RD_POS + R.RD_NEG] != 0).all())


def test_convert_refuses_bad_arguments():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 25)()
    assert lib.ctrl_pidi_convert_pdc(4, buf, 1, 1, buf) != 0
    assert lib.ctrl_pidi_convert_pdc(0, None, 1, 1, buf) != 0
    th, tw = C.c_int(), C.c_int()
    assert lib.ctrl_pidi_launch_shape(2, C.byref(th), C.byref(tw)) != 0
    for k in (0, 1):
        assert lib.ctrl_pidi_launch_shape(k, C.byref(th), C.byref(tw)) == 0 and th.value >= 8 and tw.value >= 8


def test_module_equals_the_functional_forward():
    """the torch module (on-the-fly PDC, controlnet_aux's keys) and forward() (converted kernels, the a4 / d algebra's source form) agree"""
    sd = R.make_state_dict(11, "he")
    m = R.PiDiNetRef().double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == dict(R.spec())
    fr = R.make_frames(2, 1, 64, 64)
    with torch.no_grad():
        outs = m(fr.permute(0, 3, 1, 2).double().flip(1) / 255.0)
    assert len(outs) == 5
    lg = R.forward(sd, fr)
    assert float((torch.logit(outs[-1][:, 0]) - lg).abs().max()) < 1e-9


def test_side_map_algebra():
    """MapReduce(CSAM(s)) = sigmoid(conv3x3(a4)) * d + b_red with a4 = W_att1 . relu(s) + b_att1 and d = w_red . s: what lets the
    context head write five values per pixel"""
    x, w1, b1, ws, att_w, att_b, red_w, side_w, red_b = PF.head_problem(60, 1, 16, 24, 3)
    t = F.conv2d(F.relu(x.double()), w1.double(), b1.double())
    a4, _, d, _ = R.head_context_ref(t, ws, att_w, att_b, red_w)
    e, _ = R.side_ref(a4, d, side_w, red_b)
    s = sum(F.conv2d(t, w.double(), padding=dl, dilation=dl) for w, dl in zip(ws, R.DILATIONS))
    y = torch.sigmoid(F.conv2d(F.conv2d(F.relu(s), att_w.double(), att_b.double()), side_w.double(), padding=1))
    want = F.conv2d(s * y, red_w.double(), red_b.double())
    assert float((e - want).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- the detector's check
@pytest.fixture(scope="module")
def calibrated():
    sd = R.make_state_dict(3, "calibrated")
    cases = {}
    for key, (N, H, W) in PF.DETECTOR_CASES.items():
        fr = R.make_frames(5, N, H, W)
        cases[key] = (fr,) + R.detector_tolerance(sd, fr)
    return sd, cases


def test_tolerance_is_useful_and_the_logits_spread(calibrated):
    _, cases = calibrated
    for key, (fr, ref, emu, dev, tol) in cases.items():
        print("PIDI-REF %s: logit min %.3f max %.3f std %.3f | max |emulated - fp64| %.3e, tolerance %.3e" % (
            key, float(ref.min()), float(ref.max()), float(ref.std()), dev, tol))
        assert float(ref.std()) > 0.3 and float(ref.min()) < 0 < float(ref.max())
        assert tol < 0.05 * float(ref.std())
        assert R.outside(emu, ref, tol) == 0


@pytest.mark.parametrize("planted", R.PLANTS)
def test_planted_errors_are_caught(calibrated, planted):
    """every planted error puts more than half of the pixels outside the tolerance of the whole-detector check"""
    sd, cases = calibrated
    for key, (fr, ref, emu, dev, tol) in cases.items():
        bad = R.forward(sd, fr, emulate=True, **{planted: True})
        n = R.outside(bad, ref, tol)
        print("PIDI-PLANTED %s %s: %d of %d logits outside (%.1f %%)" % (planted, key, n, ref.numel(), 100.0 * n / ref.numel()))
        assert n > ref.numel() // 2


@pytest.mark.parametrize("kind,planted", [("ad", "ad_inverted"), ("rd", "rd_first8"), ("cd", "cd_no_centre")])
def test_block_bound_catches_a_wrong_kernel(kind, planted):
    """the per-kernel bound of the GPU block test: a block computed with the planted kernel leaves it in most elements"""
    x, w1, w2, _, _ = PF.block_problem(kind, 60, 60, False, 1, 9, 17, 4)
    ref, bound = R.block_ref(x, R.convert_pdc(kind, w1.double()).float(), w2)
    bad, _ = R.block_ref(x, R._planted_kernel(kind, w1.double(), (planted,)).float(), w2)
    n = int(((bad - ref).abs() > bound).sum())
    print("PIDI-PLANTED block %s: %d of %d outside; bound max %.2e on values of deviation %.2f" % (planted, n, ref.numel(), float(bound.max()),
                                                                                                   float(ref.std())))
    assert n > ref.numel() // 2
    assert float(bound.max()) < 0.05 * float(ref.std())


def test_fuse_bound_catches_align_corners_and_the_interval_is_narrow():
    import hed_ref as HR
    g = torch.Generator().manual_seed(0)
    es = [torch.randn((1, 64 >> k, 64 >> k), generator=g) for k in range(4)]
    cw, cb = [0.3, -0.25, 0.2, 0.25], 0.1
    ref, bound = R.fuse_ref(es, cw, cb, 64, 64)
    bad = sum(w * F.interpolate(e.double()[:, None], (64, 64), mode="bilinear", align_corners=True)[:, 0] for e, w in zip(es, cw)) + cb
    assert int(((bad - ref).abs() > bound).sum()) > ref.numel() // 2
    lo, hi = HR.u8_interval(ref.numpy(), bound.numpy())
    assert int((hi - lo).max()) <= 1


# ---------------------------------------------------------------------------------------------------------------- pin
def test_pin_net_and_detector_to_controlnet_aux():
    aux = pytest.importorskip("controlnet_aux")
    from controlnet_aux.pidi.model import pidinet
    sd = R.make_state_dict(11, "he")
    net = pidinet().float().eval()
    net.load_state_dict(sd)
    mine = R.PiDiNetRef().eval()
    mine.load_state_dict(sd)
    frames = R.make_frames(2, 1, 128, 128)
    x = frames.permute(0, 3, 1, 2).float().flip(1) / 255.0
    with torch.no_grad():
        a, b = net(x), mine(x)
    for p, q in zip(a, b):
        assert torch.allclose(p, q, atol=1e-6)
    det = aux.PidiNetDetector(net)
    img = frames[0].numpy()
    soft = det(img, detect_resolution=128, image_resolution=128, output_type="np")
    assert np.abs(np.asarray(soft)[..., 0].astype(int) - R.detector_u8(torch.logit(b[-1][0, 0]).numpy()).astype(int)).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- ABI and refusals
def test_abi_symbols_present():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_pidi_create", "ctrl_pidi_forward", "ctrl_pidi_destroy", "ctrl_pidi_ws_bytes", "ctrl_pidi_convert_pdc",
                 "ctrl_pidi_launch_shape", "ctrl_op_pidi_stem", "ctrl_op_pidi_block", "ctrl_op_pidi_head_reduce", "ctrl_op_pidi_head_context",
                 "ctrl_op_pidi_side", "ctrl_op_pidi_fuse"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert C.sizeof(_lib.PidiConfig) == 16
    assert lib.ctrl_abi_version() == _lib.ABI_VERSION == 11


def test_python_entry_refuses_what_it_cannot_do():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import pidinet
    assert P.PidiNetDetector is pidinet.PidiNetDetector
    assert pidinet.pidinet_state_dict_spec() == [(n, tuple(s)) for n, s in R.spec()]
    det = object.__new__(P.PidiNetDetector)          # no GPU here: the refusals come before anything touches the plan
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
    with pytest.raises(ValueError, match="PidiNetDetector"):
        det(np.zeros((512, 512, 4), np.uint8))
    with pytest.raises(ValueError):
        det(img.astype(np.float32))
    with pytest.raises(ValueError):
        det(img, output_type="latent")
    with pytest.raises(ValueError, match="uint8"):
        det.run(torch.zeros((1, 64, 64, 3)))
    with pytest.raises(ValueError, match="live on"):
        det.run(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="meta"))
    det.device = torch.device("cuda:0")
    assert det.to("cuda") is det and det.to("cuda:0") is det
    with pytest.raises(ValueError):
        det.to("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.PidiNetDetector(R.make_state_dict(1))
    with pytest.raises(FileNotFoundError, match="local files only"):
        P.PidiNetDetector.from_pretrained("/nonexistent/annotators")


def test_extract_dispatches_on_the_detector(monkeypatch):
    """extract_softedge / extract_scribble hand a PidiNetDetector its own call, an HEDdetector what it got before, and refuse anything else"""
    import ctrl_adapter_amd as P
    img = np.zeros((64, 64, 3), np.uint8)
    for fn in (P.extract_softedge, P.extract_scribble):
        with pytest.raises(TypeError):
            fn([img], detector=None)
        with pytest.raises(TypeError):
            fn([img], detector=object())
    seen = []
    for cls in (P.PidiNetDetector, P.HEDdetector):
        monkeypatch.setattr(cls, "__call__", lambda self, frames, **kw: seen.append((type(self).__name__, kw)) or "out")
        det = object.__new__(cls)
        det._plan = None
        assert P.extract_softedge([img], det) == "out" and P.extract_scribble([img], det, as_pil=True) == "out"
    assert [s[0] for s in seen] == ["PidiNetDetector"] * 2 + ["HEDdetector"] * 2
    for name, kw in seen[::2]:
        assert kw == dict(detect_resolution=64, image_resolution=64, scribble=False, output_type="pt")
    for name, kw in seen[1::2]:
        assert kw == dict(detect_resolution=64, image_resolution=64, scribble=True, output_type="pil")
    assert "PiDiNet" in P.extract_softedge.__doc__ and "ctrl_helper.py:103-107" in P.extract_softedge.__doc__
