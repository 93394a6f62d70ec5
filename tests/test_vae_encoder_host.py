"""KL-VAE encoder, host side (no GPU): the parameter inventory against the restatement's diffusers keys (tests/vae_encoder_ref.py),
legacy attention names, decoder keys, unsupported configurations, the C config's layout, the new symbols, the restatement's Downsample2D
and posterior formulas, and encode_svd_image_latents / prepare_i2vgen_image_latents run with the restatement as the VAE."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT
from vae_encoder_ref import SD_VAE, TINY, DiagonalGaussianRef, DownsampleRef, VaeEncoderRef, i2vgen_prepare_image_latents
from vae_encoder_ref import seeded_pixels, svd_encode_vae_image


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("cfg", [SD_VAE, TINY], ids=["sd_vae", "tiny"])
def test_param_spec_equals_diffusers_keys(cfg):
    import ctrl_adapter_amd as P
    with torch.device("meta"):
        ref = VaeEncoderRef(**cfg)
    m = P.AutoencoderKLEncoder(**cfg)
    assert _shapes(m.state_dict()) == _shapes(ref.state_dict())


def test_default_config_key_list():
    import ctrl_adapter_amd as P
    m = P.AutoencoderKLEncoder()
    sd = _shapes(m.state_dict())
    assert len(sd) == 108
    assert sd["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert sd["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert sd["encoder.down_blocks.2.downsamplers.0.conv.weight"] == (512, 512, 3, 3)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sd
    assert sd["encoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert sd["encoder.mid_block.attentions.0.group_norm.bias"] == (512,)
    assert sd["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert sd["quant_conv.weight"] == (8, 8, 1, 1)


def _seeded_tiny():
    from ctrl_adapter_amd.synthetic import seeded_init
    return seeded_init(VaeEncoderRef(**TINY), seed=11)


def test_legacy_attention_names_and_decoder_keys():
    import ctrl_adapter_amd as P
    ref = _seeded_tiny()
    sd = ref.state_dict()
    legacy = {}
    names = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    for k, v in sd.items():
        for new, old in names.items():
            pre = "encoder.mid_block.attentions.0.%s." % new
            if k.startswith(pre):
                k = "encoder.mid_block.attentions.0.%s.%s" % (old, k[len(pre):])
                if k.endswith("weight") and old == "query":
                    v = v[:, :, None, None]          # the oldest checkpoints: 1 x 1 conv weights
                break
        legacy[k] = v
    legacy["decoder.conv_in.weight"] = torch.zeros(4, 4, 3, 3)
    legacy["post_quant_conv.weight"] = torch.zeros(4, 4, 1, 1)
    a, b = P.AutoencoderKLEncoder(**TINY), P.AutoencoderKLEncoder(**TINY)
    a.load_state_dict(sd)
    b.load_state_dict(legacy)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_save_pretrained_round_trip(tmp_path):
    import ctrl_adapter_amd as P
    ref = _seeded_tiny()
    m = P.AutoencoderKLEncoder(**TINY)
    m.load_state_dict(ref.state_dict())
    m.save_pretrained(str(tmp_path), safe_serialization=False)
    m2 = P.AutoencoderKLEncoder.from_pretrained(str(tmp_path))
    assert set(m2.state_dict()) == set(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k


@pytest.mark.parametrize("kw,field", [
    (dict(in_channels=4), "in_channels"),
    (dict(down_block_types=("DownEncoderBlock2D", "AttnDownEncoderBlock2D")), "down_block_types"),
    (dict(norm_num_groups=16), "norm_num_groups"),
    (dict(block_out_channels=(48, 64)), "block_out_channels"),
    (dict(block_out_channels=(32, 4096)), "block_out_channels"),
    (dict(latent_channels=16), "latent_channels"),
    (dict(use_quant_conv=False), "use_quant_conv"),
])
def test_unsupported_configs_raise(kw, field):
    import ctrl_adapter_amd as P
    cfg = dict(TINY)
    cfg["down_block_types"] = ("DownEncoderBlock2D",) * len(kw.get("block_out_channels", cfg["block_out_channels"]))
    cfg.update(kw)
    with pytest.raises(ValueError, match=field):
        P.AutoencoderKLEncoder(**cfg)


def test_config_struct_matches_header():
    from ctrl_adapter_amd import _lib
    src = '#include "ctrl_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu\\n", sizeof(ctrl_vae_encoder_config), sizeof(ctrl_igemm_desc));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    assert [int(v) for v in out] == [ctypes.sizeof(_lib.VaeEncoderConfig), ctypes.sizeof(_lib.IGemmDesc)]
    assert _lib.IGemmDesc.tap_origin.offset == _lib.IGemmDesc.Ktot.offset + 4


def test_new_symbols_resolve():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_vae_encoder_param_count", "ctrl_vae_encoder_param_spec", "ctrl_vae_encoder_create", "ctrl_vae_encoder_destroy",
                 "ctrl_vae_encoder_forward", "ctrl_op_vae_row_softmax", "ctrl_op_vae_posterior"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_restated_downsample_is_pad_then_stride2_conv():
    g = torch.Generator().manual_seed(0)
    d = DownsampleRef(32)
    x = torch.randn(2, 32, 10, 14, generator=g)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), d.conv.weight, d.conv.bias, stride=2)
    got = d(x)
    assert got.shape == (2, 32, 5, 7)
    assert torch.equal(got, want)
    # output pixel o reads input rows / cols 2o .. 2o + 2 (the last one past the map is zero)
    x2 = torch.zeros(1, 32, 4, 4)
    x2[0, :, 0, 0] = 1.0
    w = torch.zeros(32, 32, 3, 3)
    w[:, :, 0, 0] = 1.0
    y = F.conv2d(F.pad(x2, (0, 1, 0, 1)), w, None, stride=2)
    assert y[0, 0, 0, 0] == 32.0 and y[0, 0].sum() == 32.0


def test_posterior_clamp_and_formulas():
    g = torch.Generator().manual_seed(1)
    mean = torch.randn(2, 4, 3, 5, generator=g)
    logvar = torch.tensor([-100.0, -30.0, 0.0, 20.0, 50.0]).view(1, 1, 1, 5).expand(2, 4, 3, 5)
    d = DiagonalGaussianRef(torch.cat([mean, logvar], 1))
    assert torch.equal(d.mode(), mean)
    assert d.logvar.min() == -30.0 and d.logvar.max() == 20.0
    assert torch.allclose(d.std, torch.exp(0.5 * d.logvar)) and torch.allclose(d.var, torch.exp(d.logvar))
    gen = torch.Generator().manual_seed(5)
    s = d.sample(gen)
    eps = torch.randn(mean.shape, generator=torch.Generator().manual_seed(5))
    assert torch.equal(s, mean + d.std * eps)


class _ConstVae:
    """stand-in VAE: latents of image i are filled with i + 1 (mode) / i + 1 + noise (sample)"""

    def __init__(self):
        self.config = {"scaling_factor": 0.5}
        self.ref = None

    def encode(self, x):
        N = x.shape[0]
        mean = torch.arange(1, N + 1, dtype=torch.float32).view(N, 1, 1, 1).expand(N, 4, x.shape[2] // 8, x.shape[3] // 8)
        return type("O", (), {"latent_dist": DiagonalGaussianRef(torch.cat([mean, torch.full_like(mean, -30.0)], 1))})()


def test_svd_helper_order_with_restatement():
    import ctrl_adapter_amd as P
    vae = _ConstVae()
    img = torch.zeros(2, 3, 16, 24)
    got = P.encode_svd_image_latents(vae, img, "cpu", 3, True)
    assert got.shape == (12, 4, 2, 3)
    per = got[:, 0, 0, 0].tolist()
    assert per == [0, 0, 1, 2] * 3            # zero negatives first, then the images; repeat tiles the whole batch
    assert torch.equal(got, svd_encode_vae_image(vae, img, "cpu", 3, True))
    assert P.encode_svd_image_latents(vae, img, "cpu", 1, False)[:, 0, 0, 0].tolist() == [1, 2]


def test_i2vgen_helper_mask_and_layout_with_restatement():
    import ctrl_adapter_amd as P
    torch.manual_seed(0)
    ref = _seeded_tiny().eval()
    img = seeded_pixels(2, 16, 16, seed=2)
    F_ = 5
    got = P.prepare_i2vgen_image_latents(ref, img, "cpu", F_, 2, True, generator=torch.Generator().manual_seed(7))
    want = i2vgen_prepare_image_latents(ref, img, "cpu", F_, 2, True, generator=torch.Generator().manual_seed(7))
    assert got.shape == (8, 4, F_, 8, 8)
    assert torch.equal(got, want)
    for f in range(1, F_):
        assert torch.all(got[:, :, f] == f / (F_ - 1))
    assert torch.equal(got[:4], got[4:])                                     # CFG duplicates the whole batch
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])  # repeat tiles the images


def test_forward_without_gpu_raises():
    import ctrl_adapter_amd as P
    m = P.AutoencoderKLEncoder(**TINY)
    with pytest.raises(RuntimeError):
        m.encode(torch.zeros(1, 3, 16, 16))
