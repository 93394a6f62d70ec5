"""CLIP vision tower, host side (no GPU): the parameter inventory against transformers' CLIPVisionModelWithProjection, the fp32
restatement (tests/clip_vision_ref.py) against tests/golden/clip_vision.pt, SVD's preprocessing restatement against the pipeline's own
helpers (the same golden), transformers' file layout through from_pretrained, the encode_svd_image / encode_i2vgen_image logic with a
stand-in encoder, and the new C symbols."""
import os

import numpy as np
import pytest
import torch

from clip_vision_ref import TINY, VIT_H, CLIPVisionRef, gaussian_taps, resize_with_antialiasing, seeded_pixels
from helpers import check_digest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_vision.pt")


def _golden():
    return torch.load(GOLDEN, weights_only=False)


def _hf_config(cfg):
    from transformers import CLIPVisionConfig
    return CLIPVisionConfig(hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"], projection_dim=cfg["projection_dim"],
                            num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                            image_size=cfg["image_size"], patch_size=cfg["patch_size"], hidden_act=cfg["hidden_act"],
                            layer_norm_eps=cfg["layer_norm_eps"])


def _seeded(cfg):
    import ctrl_adapter_amd.synthetic as syn
    from make_clip_vision_golden import WEIGHT_SEED
    return syn.seeded_init(CLIPVisionRef(**cfg), seed=WEIGHT_SEED).eval()


@pytest.mark.parametrize("cfg", [TINY, VIT_H], ids=["tiny", "vit_h"])
def test_param_spec_equals_transformers_state_dict(cfg):
    pytest.importorskip("transformers")
    from transformers import CLIPVisionModelWithProjection as HF
    import ctrl_adapter_amd as P
    with torch.device("meta"):
        hf = HF(_hf_config(cfg))
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    m = P.CLIPVisionModelWithProjection(**cfg)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    ref = {k: tuple(v.shape) for k, v in CLIPVisionRef(**dict(cfg, num_hidden_layers=1)).state_dict().items()}
    assert set(ref) <= set(want)


@pytest.mark.parametrize("bad", [dict(hidden_act="relu"), dict(num_attention_heads=3), dict(hidden_size=4096, num_attention_heads=32),
                                 dict(image_size=50), dict(image_size=448, patch_size=14), dict(num_channels=1)])
def test_unsupported_configs_are_value_errors(bad):
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError):
        P.CLIPVisionModelWithProjection(**dict(TINY, **bad))


@pytest.mark.parametrize("act", ["quick", "gelu"])
def test_restatement_matches_transformers_tiny(act):
    g = _golden()
    cfg = dict(TINY, hidden_act="quick_gelu" if act == "quick" else "gelu")
    rec = g["tiny_" + act]
    px = seeded_pixels(rec["N"], cfg["image_size"], seed=rec["pixels_seed"])
    with torch.no_grad():
        r = _seeded(cfg)(px, output_hidden_states=True)
    for name, t in (("image_embeds", r.image_embeds), ("last", r.last_hidden_state), ("penultimate", r.hidden_states[-2])):
        torch.testing.assert_close(t, rec[name]["full"], rtol=1e-5, atol=1e-5, msg=name)


def test_restatement_matches_transformers_vit_h_two_layers():
    g = _golden()
    rec = g["vith"]
    px = seeded_pixels(rec["N"], g["vith_cfg"]["image_size"], seed=rec["pixels_seed"])
    with torch.no_grad():
        r = _seeded(g["vith_cfg"])(px, output_hidden_states=True)
    check_digest(r.image_embeds, rec["image_embeds"], 1e-5, "image_embeds")
    check_digest(r.last_hidden_state, rec["last"], 1e-5, "last")
    check_digest(r.hidden_states[-2], rec["penultimate"], 1e-5, "penultimate")


def test_resize_restatement_matches_the_pipeline_helpers():
    for case in _golden()["resize"]:
        g = torch.Generator().manual_seed(case["seed"])
        u8 = torch.randint(0, 256, (1, case["H"], case["W"], 3), generator=g, dtype=torch.uint8)
        assert int(u8.long().sum()) == case["input_sum"]
        x = u8.float().div(255.0).permute(0, 3, 1, 2).contiguous()
        y = resize_with_antialiasing(x * 2.0 - 1.0, (224, 224))
        d = case["out"]
        s = y.reshape(-1)[::d["step"]][:4096]
        err = (s - d["samples"]).abs().max().item()
        assert err <= 2e-6, "%dx%d: %.3e" % (case["H"], case["W"], err)


def test_gaussian_rule():
    # skimage's sigma, 2 sigma each side, odd, at least 3, the 0.001 floor
    assert gaussian_taps(576, 224)[1] == 3 and gaussian_taps(1024, 224)[1] == 7
    sigma, ks, w = gaussian_taps(224, 224)
    assert sigma == 0.001 and ks == 3 and w[1] == 1.0
    assert gaussian_taps(1120, 224)[1] == 9     # int(max(8.0, 3)) = 8 -> bumped to odd


@pytest.mark.parametrize("variant", [None, "fp16"])
def test_from_pretrained_reads_transformers_layout(tmp_path, variant):
    pytest.importorskip("transformers")
    from transformers import CLIPVisionModelWithProjection as HF
    import ctrl_adapter_amd as P
    cfg = dict(TINY, num_hidden_layers=1)
    hf = HF(_hf_config(cfg)).eval()
    if variant:
        hf = hf.half()
    d = tmp_path / "ckpt"
    hf.save_pretrained(str(d / "image_encoder"), variant=variant)
    m = P.CLIPVisionModelWithProjection.from_pretrained(str(d), subfolder="image_encoder", variant=variant,
                                                        torch_dtype=torch.float16 if variant else None)
    assert next(m.parameters()).dtype == (torch.float16 if variant else torch.float32)
    assert m.config.image_size == 56 and m.config.patch_size == 14 and m.config.hidden_act == "quick_gelu"
    want = {k: v for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    got = m.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k].to(v.dtype), v), k


class _FakeEncoder(torch.nn.Module):
    """records the pixels it is given; image_embeds[n] = [mean of image n, n, ...]"""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, dtype=dtype))
        self.seen = []

    def forward(self, pixel_values):
        self.seen.append(pixel_values)
        N = pixel_values.shape[0]
        e = torch.zeros(N, 4, dtype=pixel_values.dtype)
        e[:, 0] = pixel_values.float().reshape(N, -1).mean(1).to(e.dtype)
        e[:, 1] = torch.arange(N, dtype=e.dtype)

        class O:
            image_embeds = e
        return O()


class _FE:
    image_mean = [0.5, 0.25, 0.125]
    image_std = [0.5, 0.5, 2.0]


@pytest.mark.parametrize("cfg_guidance", [False, True])
def test_encode_repeat_order_and_zero_negatives(cfg_guidance):
    import ctrl_adapter_amd as P
    enc = _FakeEncoder()
    img = torch.rand(2, 3, 8, 8)
    out = P.encode_i2vgen_image(enc, _FE(), img, "cpu", 3, cfg_guidance)
    assert out.shape == ((12 if cfg_guidance else 6), 1, 4)
    pos = out[6:] if cfg_guidance else out
    assert pos[:, 0, 1].tolist() == [0, 0, 0, 1, 1, 1]              # image-major, as the pipelines' repeat + view
    if cfg_guidance:
        assert torch.count_nonzero(out[:6]) == 0
    assert torch.equal(enc.seen[0], img)                            # tensors reach the encoder un-normalised (I2VGen-XL)


def test_encode_svd_tensor_is_normalised_without_resize():
    import ctrl_adapter_amd as P
    enc = _FakeEncoder()
    img = torch.rand(1, 3, 8, 8)
    P.encode_svd_image(enc, _FE(), img, "cpu", 1, False)
    m = torch.tensor(_FE.image_mean).view(1, 3, 1, 1)
    s = torch.tensor(_FE.image_std).view(1, 3, 1, 1)
    assert enc.seen[0].shape == (1, 3, 8, 8)
    torch.testing.assert_close(enc.seen[0], (img - m) / s, rtol=0, atol=0)


def test_encode_i2vgen_pil_is_rescaled_and_normalised():
    PIL = pytest.importorskip("PIL.Image")
    import ctrl_adapter_amd as P
    arr = np.random.default_rng(3).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    enc = _FakeEncoder(torch.float16)
    out = P.encode_i2vgen_image(enc, None, PIL.fromarray(arr), "cpu", 1, True)
    assert out.dtype == torch.float16 and out.shape == (2, 1, 4)
    x = torch.from_numpy(arr.astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    m = torch.tensor(P.vision_encoder.OPENAI_CLIP_MEAN).view(1, 3, 1, 1)
    s = torch.tensor(P.vision_encoder.OPENAI_CLIP_STD).view(1, 3, 1, 1)
    assert enc.seen[0].dtype == torch.float16
    torch.testing.assert_close(enc.seen[0], ((x - m) / s).half(), rtol=0, atol=0)


def test_encode_rejects_non_rgb():
    PIL = pytest.importorskip("PIL.Image")
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError):
        P.encode_i2vgen_image(_FakeEncoder(), None, PIL.new("L", (8, 8)), "cpu", 1, False)


def test_mirror_forward_needs_the_gpu():
    import ctrl_adapter_amd as P
    m = P.CLIPVisionModelWithProjection(**TINY)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 56, 56))


def test_vision_abi_symbols_resolve():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_vision_encoder_param_count", "ctrl_vision_encoder_param_spec", "ctrl_vision_encoder_create",
                 "ctrl_vision_encoder_destroy", "ctrl_vision_encoder_forward", "ctrl_op_vision_patchify", "ctrl_op_vision_embed",
                 "ctrl_op_vision_cls_ln", "ctrl_op_clip_resize_aa"):
        assert hasattr(lib, name), name
    assert lib.ctrl_abi_version() == 11
    cfg = _lib.VisionEncoderConfig()
    cfg.image_size, cfg.patch_size, cfg.hidden_size, cfg.intermediate_size = 224, 14, 1280, 5120
    cfg.num_hidden_layers, cfg.num_attention_heads, cfg.projection_dim, cfg.hidden_act, cfg.layer_norm_eps = 32, 16, 1024, 1, 1e-5
    import ctypes
    assert lib.ctrl_vision_encoder_param_count(ctypes.byref(cfg)) == 5 + 32 * 16 + 3
    cfg.num_attention_heads = 20                 # head_dim 64 ok
    assert lib.ctrl_vision_encoder_param_count(ctypes.byref(cfg)) > 0
    cfg.num_attention_heads = 10                 # head_dim 128: refused
    assert lib.ctrl_vision_encoder_param_count(ctypes.byref(cfg)) == -1
