"""The lineart annotator without a GPU: tests/lineart_ref.py against torch's own layers, the two GEMM-form identities the plan relies on
(a transposed convolution as four phase convolutions, a reflection-padded 3x3 as a valid convolution over a map whose border the producer
wrote), the byte rule, the planted errors against the checks of tests/test_gpu_lineart.py, the refusals of the Python entry, and the pin
to controlnet_aux wherever that package exists."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers  # noqa: F401
import lineart_ref as R


@pytest.fixture(scope="module")
def calibrated():
    sd = R.make_state_dict(3, "calibrated")
    fr = R.make_frames(5, 1, 64, 64)
    return (sd, fr) + R.detector_tolerance(sd, fr)


# ---------------------------------------------------------------------------------------------------------------- restatement == torch
def test_restatement_equals_torchs_own_layers():
    """the functional forward against an nn.Sequential stack of ReflectionPad2d, Conv2d, InstanceNorm2d, ConvTranspose2d and Sigmoid"""
    sd = R.make_state_dict(7, "plain")
    net = R.GeneratorRef().double().eval()
    net.load_state_dict({k: v.double() for k, v in sd.items()})          # strict: the keys are the module's own
    assert [k for k, _ in R.spec()] == list(net.state_dict().keys())
    assert all(isinstance(m, torch.nn.InstanceNorm2d) and not m.affine and not m.track_running_stats and m.eps == 1e-5
               for m in net.modules() if "Norm" in type(m).__name__)
    for H, W in ((64, 64), (64, 128)):
        fr = R.make_frames(H + W, 2, H, W)
        x = fr.permute(0, 3, 1, 2).double() / 255.0
        with torch.no_grad():
            want, line = net.logits(x)[:, 0], net(x)[:, 0]
        got = R.forward(sd, fr)
        assert float((got - want).abs().max()) < 1e-10
        assert float((torch.sigmoid(got) - line).abs().max()) < 1e-10


def test_calibrated_checkpoint_and_tolerance(calibrated):
    sd, fr, ref, emu, dev, tol = calibrated
    std = float(ref.std())
    print("LINEART-HOST logits std %.3f; emulated deviation %.3e, tolerance %.3e" % (std, dev, tol))
    assert 1.0 < std < 3.0
    assert len(np.unique(R.detector_u8(ref.float().numpy()))) > 20
    assert tol < 0.1 * std and R.outside(emu, ref, tol) == 0


def test_dropped_biases_cancel():
    """two state dicts that differ only in the biases in front of an InstanceNorm: the fp64 restatement, which keeps them, gives the same
    logits to rounding"""
    a, b = R.make_state_dict(3, "calibrated"), R.make_state_dict(3, "calibrated", bias_seed=8)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert sorted(differ) == sorted(k for k, _ in R.spec() if k.endswith(".bias") and k != "model4.1.bias")
    fr = R.make_frames(5, 1, 64, 64)
    assert float((R.forward(a, fr) - R.forward(b, fr)).abs().max()) < 1e-9
    assert torch.equal(R.forward(a, fr, emulate=True), R.forward(b, fr, emulate=True))


# ---------------------------------------------------------------------------------------------------------------- the two GEMM forms
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (4, 4), (7, 2)])
@pytest.mark.parametrize("Ci,Co", [(8, 6), (5, 9)])
def test_transposed_conv_is_four_phase_convs(H, W, Ci, Co):
    g = torch.Generator().manual_seed(H * 10 + W + Ci)
    x = torch.randn((2, Ci, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Ci, Co, 3, 3), generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    got = R.convT_by_phases(x, R.pack_convT_phase(w))
    assert got.shape == want.shape == (2, Co, 2 * H, 2 * W)
    assert float((got - want).abs().max()) < 1e-12
    if H * W > 1:
        wrong = R.convT_by_phases(x, R.pack_convT_phase(w, planted=True))
        assert float((wrong - want).abs().max()) > 0.1            # weights read as [Cout][Cin]


def test_phase_pack_has_zeros_in_the_unused_taps():
    w = torch.ones(4, 3, 3, 3, dtype=torch.float64)
    p = R.pack_convT_phase(w)
    used = p.abs().sum(dim=(1, 3)) > 0                            # [phase][tap]
    assert used.tolist() == [[False, False, False, True], [False, False, True, True], [False, True, False, True], [True, True, True, True]]


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (16, 16)])
def test_valid_conv_over_reflect_padded_map(H, W):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn((2, 6, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((4, 6, 3, 3), generator=g, dtype=torch.float64)
    want = torch.nn.Sequential(torch.nn.ReflectionPad2d(1))(x)
    xp = R.reflect_pad(x, 1)
    assert torch.equal(xp, want) and torch.equal(xp[:, :, 1:-1, 1:-1], x)
    assert torch.equal(xp[:, :, 0], xp[:, :, 2]) and torch.equal(xp[:, :, :, -1], xp[:, :, :, -3])      # no edge repeat
    ref, _ = R.conv_valid_ref(xp, w)
    assert float((ref - F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)).abs().max()) == 0
    assert float((ref - F.conv2d(x, w, padding=1)).abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_byte_rule_truncates_then_inverts():
    z = np.array([-8.0, -1.0, 0.0, 0.0078, 1.0, 8.0], dtype=np.float32)
    got = R.detector_u8(z)
    line = 1 / (1 + np.exp(-z.astype(np.float64)))
    assert got.dtype == np.uint8 and got.tolist() == [255 - int(np.floor(255 * v)) for v in line]
    assert got[0] == 255 and got[-1] == 1 and got[2] == 255 - 127          # 127.5 truncates to 127
    assert R.detector_u8(z, rounding=True)[2] == 255 - 128
    lo, hi = R.u8_interval(z.astype(np.float64), np.full(z.shape, 1e-4))
    assert bool(((got >= lo) & (got <= hi)).all()) and int((hi - lo).max()) <= 1


# ---------------------------------------------------------------------------------------------------------------- planted errors
@pytest.mark.parametrize("planted", ["bgr", "zero_pad", "convT_as_cout_cin"])
def test_planted_net_errors_leave_the_detector_tolerance(calibrated, planted):
    sd, fr, ref, emu, dev, tol = calibrated
    bad = R.forward(sd, fr, emulate=True, **{planted: True})
    n = R.outside(bad, ref, tol)
    print("LINEART-PLANTED %s: %d of %d logits outside (%.1f %%)" % (planted, n, ref.numel(), 100.0 * n / ref.numel()))
    assert n > ref.numel() // 2


def test_planted_byte_rules_leave_the_byte_check(calibrated):
    sd, fr, ref, emu, dev, tol = calibrated
    z = emu.float().numpy()
    bound = np.full(ref.shape, tol)
    assert R.u8_failures(R.detector_u8(z), ref.numpy(), bound) == 0
    assert R.u8_failures(R.detector_u8(z, inverted=False), ref.numpy(), bound) > ref.numel() // 2
    # rounding moves half of the bytes by one; the whole-detector interval is several bytes wide, the head kernel's own is not
    zz = torch.linspace(-4, 4, 4001, dtype=torch.float64).numpy()
    tight = np.full(zz.shape, 1e-5)
    assert R.u8_failures(R.detector_u8(zz.astype(np.float32)), zz, tight) == 0
    assert R.u8_failures(R.detector_u8(zz.astype(np.float32), rounding=True), zz, tight) > zz.size // 3


def test_stem_bound_catches_channel_order_and_padding():
    fr = R.make_frames(7, 1, 12, 20)
    fr[..., 0] = fr[..., 0] // 3
    fr[..., 2] = 255 - fr[..., 2] // 4
    w = R.make_state_dict(7, "plain")["model0.1.weight"]
    ref, bound = R.stem_ref(fr, w)
    assert float(bound.max()) < 0.01 * float(ref.std())
    assert int(((R.stem_ref(fr, w, bgr=True)[0] - ref).abs() > bound).sum()) > ref.numel() // 2
    border = torch.ones_like(ref, dtype=torch.bool)
    border[:, :, 3:-3, 3:-3] = False
    zp = (R.stem_ref(fr, w, zero_pad=True)[0] - ref).abs() > bound
    assert int(zp[border].sum()) > int(border.sum()) // 2 and int(zp[~border].sum()) == 0


def test_apply_bound_catches_unbiased_variance():
    """at the sizes the GPU test uses (5 x 7, 1 x 9) the unbiased variance moves every value by 1.5 % and more; the bound is one fp16 store"""
    g = torch.Generator().manual_seed(1)
    for H, W in ((5, 7), (1, 9)):
        x = (torch.randn((2, 64, H, W), generator=g) * 1.5 + 0.3).half()
        s, _, q, _ = R.in_stats_ref(x)
        stats = torch.stack([s, q], dim=-1).float()
        ref, bound = R.in_apply_ref(x, stats, relu=False)
        bad, _ = R.in_apply_ref(x, stats, relu=False, unbiased=True)
        want = F.instance_norm(x.double(), eps=1e-5)
        assert float((ref - want).abs().max()) < 1e-5          # (the stats were rounded to fp32)
        n = int(((bad - ref).abs() > bound).sum())
        assert n > ref.numel() // 2, (H, W, n)


# ---------------------------------------------------------------------------------------------------------------- pin
def test_pin_net_and_detector_to_controlnet_aux():
    aux = pytest.importorskip("controlnet_aux")
    from controlnet_aux.lineart import Generator
    sd = R.make_state_dict(11, "calibrated")
    net = Generator(3, 1, 3).float().eval()
    net.load_state_dict(sd)
    mine = R.GeneratorRef().eval()
    mine.load_state_dict(sd)
    frames = R.make_frames(2, 1, 128, 128)
    x = frames.permute(0, 3, 1, 2).float() / 255.0
    with torch.no_grad():
        a, b = net(x), mine(x)
        lg = mine.logits(x)[0, 0]
    assert torch.allclose(a, b, atol=1e-6)
    det = aux.LineartDetector(net, net)
    out = det(frames[0].numpy(), detect_resolution=128, image_resolution=128, output_type="np")
    assert np.abs(np.asarray(out)[..., 0].astype(int) - R.detector_u8(lg.numpy()).astype(int)).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- ABI and refusals
def test_abi_symbols_present():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    header = open(helpers.ROOT + "/include/ctrl_hip.h").read()
    for name in ("ctrl_lineart_create", "ctrl_lineart_forward", "ctrl_lineart_destroy", "ctrl_lineart_ws_bytes", "ctrl_lineart_launch_shape",
                 "ctrl_op_lineart_stem", "ctrl_op_in_stats_ws_floats", "ctrl_op_in_stats", "ctrl_op_in_apply", "ctrl_op_lineart_head",
                 "ctrl_op_pack_convt_w_phase", "ctrl_op_pack_convt_w_phase_ovf"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header, name
    assert C.sizeof(_lib.LineartConfig) == 16
    assert lib.ctrl_abi_version() == _lib.ABI_VERSION == 11          # symbols were added, nothing changed
    a, b = C.c_int(), C.c_int()
    for k in (0, 1):
        assert lib.ctrl_lineart_launch_shape(k, 0, C.byref(a), C.byref(b)) == 0 and a.value >= 1 and b.value >= 4
    for Cw in (64, 128, 256):
        assert lib.ctrl_lineart_launch_shape(2, Cw, C.byref(a), C.byref(b)) == 0 and a.value * Cw == 32768
    assert lib.ctrl_lineart_launch_shape(3, 64, C.byref(a), C.byref(b)) != 0 and lib.ctrl_lineart_launch_shape(2, 48, C.byref(a), C.byref(b)) != 0
    assert lib.ctrl_op_in_stats_ws_floats(2, 4096, 64) == 2 * 8 * 2 * 64 and lib.ctrl_op_in_stats_ws_floats(1, 1, 256) == 512
    assert lib.ctrl_op_in_stats_ws_floats(1, 16, 48) == 0


def test_op_entries_refuse_before_any_device_is_touched():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)
    assert lib.ctrl_op_lineart_stem(p, 1, 3, 8, p, p, None, None) != 0 and b"at least 4" in lib.ctrl_last_error()
    assert lib.ctrl_op_in_apply(p, p, 1, 1, 8, 64, 1e-5, 0, None, 0, 1, p, None, None) != 0 and b"above p" in lib.ctrl_last_error()
    assert lib.ctrl_op_in_apply(p, p, 1, 8, 8, 64, 1e-5, 0, None, 0, 2, p, None, None) != 0
    assert lib.ctrl_op_in_apply(p, p, 1, 8, 8, 72, 1e-5, 0, None, 0, 0, p, None, None) != 0
    assert lib.ctrl_op_in_stats(p, 1, 16, 24, p, p, None) != 0
    assert lib.ctrl_op_lineart_head(p, 1, 8, 8, p, 0.0, 2, p, None, None) != 0 and b"out_channels" in lib.ctrl_last_error()
    assert lib.ctrl_op_pack_convt_w_phase(p, 5, p, 64, 64, None) != 0
    assert lib.ctrl_lineart_forward(None, p, 1, 64, 64, 0, 3, p, None, 0, None) != 0 and b"null plan" in lib.ctrl_last_error()
    assert lib.ctrl_lineart_ws_bytes(None, 1, 64, 64, 0) == 0


def test_python_entry_refuses_what_it_cannot_do():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import lineart
    assert P.LineartDetector is lineart.LineartDetector and P.extract_lineart is lineart.extract_lineart
    assert lineart.lineart_state_dict_spec() == [(n, tuple(s)) for n, s in R.spec()] and P.lineart_state_dict_spec is lineart.lineart_state_dict_spec
    sd = R.make_state_dict(1, "plain")
    # key and shape refusals come before the device is looked at
    with pytest.raises(KeyError, match="model2.1.conv_block.5.bias"):
        P.LineartDetector({k: v for k, v in sd.items() if k != "model2.1.conv_block.5.bias"})
    with pytest.raises(KeyError, match="coarse"):
        P.LineartDetector(sd, {k: v for k, v in sd.items() if k != "model0.1.bias"})
    with pytest.raises(ValueError, match="model3.0.weight"):                 # the transposed layout is [Cin][Cout]
        P.LineartDetector(dict(sd, **{"model3.0.weight": sd["model3.0.weight"].permute(1, 0, 2, 3).contiguous()}))
    with pytest.raises(ValueError, match="model1.0.bias"):
        P.LineartDetector(dict(sd, **{"model1.0.bias": torch.zeros(64)}))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.LineartDetector({"module." + k: v for k, v in sd.items()})
    det = object.__new__(P.LineartDetector)          # no GPU here: the refusals come before anything touches the plan
    det._plan = None
    det.device = torch.device("cpu")
    det.has_coarse = False
    img = np.zeros((512, 512, 3), np.uint8)
    with pytest.raises(ValueError, match="coarse"):
        det(img, coarse=True)
    with pytest.raises(ValueError, match="coarse"):
        det.run(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), coarse=True)
    with pytest.raises(ValueError, match="resized"):
        det(np.zeros((480, 512, 3), np.uint8))
    with pytest.raises(ValueError, match="resized"):
        det(img, detect_resolution=384)
    with pytest.raises(ValueError, match="resized"):
        det(np.zeros((512, 768, 3), np.uint8), image_resolution=768)
    with pytest.raises(ValueError, match="one size"):
        det([img, np.zeros((512, 576, 3), np.uint8)])
    with pytest.raises(ValueError, match="LineartDetector"):
        det(np.zeros((512, 512, 4), np.uint8))
    with pytest.raises(ValueError):
        det(img.astype(np.float32))
    with pytest.raises(ValueError):
        det(img, output_type="latent")
    with pytest.raises(ValueError, match="uint8"):
        det.run(torch.zeros((1, 64, 64, 3)))
    with pytest.raises(ValueError, match="channels"):
        det.run(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), channels=2)
    with pytest.raises(ValueError, match="live on"):
        det.run(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="meta"))
    det.device = torch.device("meta")
    with pytest.raises(ValueError, match="multiples of 64"):
        det.run(torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match="frames_per_group"):
        det.run(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="meta"), frames_per_group=0)
    det.device = torch.device("cuda:0")
    assert det.to("cuda") is det and det.to("cuda:0") is det
    with pytest.raises(ValueError):
        det.to("cpu")
    with pytest.raises(FileNotFoundError, match="local files only"):
        P.LineartDetector.from_pretrained("/nonexistent/annotators")


def test_from_pretrained_reads_local_files_only(tmp_path, monkeypatch):
    import ctrl_adapter_amd as P
    sd, sd2 = R.make_state_dict(1, "plain"), R.make_state_dict(2, "plain")
    seen = []
    monkeypatch.setattr(P.LineartDetector, "__init__", lambda self, a, b=None, **kw: seen.append((a, b)))
    torch.save(sd, tmp_path / "sk_model.pth")
    P.LineartDetector.from_pretrained(tmp_path)
    assert seen[-1][1] is None and torch.equal(seen[-1][0]["model4.1.weight"], sd["model4.1.weight"])
    torch.save({"state_dict": sd2}, tmp_path / "sk_model2.pth")
    P.LineartDetector.from_pretrained(str(tmp_path))
    assert torch.equal(seen[-1][1]["model4.1.weight"], sd2["model4.1.weight"])
    P.LineartDetector.from_pretrained(tmp_path / "sk_model.pth")
    assert seen[-1][1] is not None
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match="no sk_model.pth under"):
        P.LineartDetector.from_pretrained(tmp_path / "empty")


def test_extract_lineart_hands_the_detector_its_own_call(monkeypatch):
    import ctrl_adapter_amd as P
    img = np.zeros((64, 128, 3), np.uint8)
    for bad in (None, object(), object.__new__(P.HEDdetector)):
        with pytest.raises(TypeError):
            P.extract_lineart([img], bad)
    seen = []
    monkeypatch.setattr(P.LineartDetector, "__call__", lambda self, frames, **kw: seen.append(kw) or "out")
    det = object.__new__(P.LineartDetector)
    det._plan = None
    assert P.extract_lineart([img], det) == "out" and P.extract_lineart([img], det, coarse=True, as_pil=True) == "out"
    assert seen == [dict(coarse=False, detect_resolution=64, image_resolution=64, output_type="pt"),
                    dict(coarse=True, detect_resolution=64, image_resolution=64, output_type="pil")]
    assert "ctrl_helper.py:190-191" in P.extract_lineart.__doc__
