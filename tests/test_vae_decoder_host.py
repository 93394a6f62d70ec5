"""KL-VAE decoder, host side (no GPU): the parameter inventory against the restatement's diffusers keys (tests/vae_decoder_ref.py), legacy
attention names, encoder keys, unsupported configurations, the temporal-decoder checkpoint, the C config's layout, the new symbols, the
restatement's Upsample2D and uint8 formulas, decode_sdxl_latents / decode_i2vgen_latents run with the restatement as the VAE, and the
whole-VAE module's keys and config."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT
from vae_decoder_ref import SD_VAE, TINY, UpsampleRef, VaeDecoderRef, VaeRef, i2vgen_decode_latents, pil_to_u8, sdxl_decode_latents
from vae_decoder_ref import seeded_latents, u8_of_sample


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("cfg", [SD_VAE, TINY], ids=["sd_vae", "tiny"])
def test_param_spec_equals_diffusers_keys(cfg):
    import ctrl_adapter_amd as P
    with torch.device("meta"):
        ref = VaeDecoderRef(**cfg)
    m = P.AutoencoderKLDecoder(**cfg)
    assert _shapes(m.state_dict()) == _shapes(ref.state_dict())


def test_default_config_key_list():
    import ctrl_adapter_amd as P
    sd = _shapes(P.AutoencoderKLDecoder().state_dict())
    assert sd["decoder.conv_in.weight"] == (512, 4, 3, 3)
    for i in range(4):
        for j in range(3):
            assert "decoder.up_blocks.%d.resnets.%d.conv1.weight" % (i, j) in sd
        assert "decoder.up_blocks.%d.resnets.3.conv1.weight" % i not in sd
    assert sd["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert sd["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert sd["decoder.up_blocks.2.upsamplers.0.conv.weight"] == (256, 256, 3, 3)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in sd
    assert sd["decoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert sd["decoder.conv_norm_out.weight"] == (128,)
    assert sd["decoder.conv_out.weight"] == (3, 128, 3, 3)
    assert sd["post_quant_conv.weight"] == (4, 4, 1, 1)
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in sd)


def _seeded_tiny(cls=VaeDecoderRef):
    from ctrl_adapter_amd.synthetic import seeded_init
    return seeded_init(cls(**TINY), seed=11)


def test_legacy_attention_names_and_encoder_keys():
    import ctrl_adapter_amd as P
    sd = _seeded_tiny().state_dict()
    legacy = {}
    names = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    for k, v in sd.items():
        for new, old in names.items():
            pre = "decoder.mid_block.attentions.0.%s." % new
            if k.startswith(pre):
                k = "decoder.mid_block.attentions.0.%s.%s" % (old, k[len(pre):])
                if k.endswith("weight") and old == "query":
                    v = v[:, :, None, None]          # the oldest checkpoints: 1 x 1 conv weights
                break
        legacy[k] = v
    legacy["encoder.conv_in.weight"] = torch.zeros(32, 3, 3, 3)
    legacy["quant_conv.weight"] = torch.zeros(8, 8, 1, 1)
    a, b = P.AutoencoderKLDecoder(**TINY), P.AutoencoderKLDecoder(**TINY)
    a.load_state_dict(sd)
    b.load_state_dict(legacy)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
        assert torch.equal(v, sd[k]), k


def test_temporal_decoder_checkpoint_is_refused():
    import ctrl_adapter_amd as P
    sd = dict(_seeded_tiny().state_dict())
    sd["decoder.up_blocks.0.resnets.0.spatial_res_block.conv1.weight"] = torch.zeros(64, 64, 3, 3)
    with pytest.raises(ValueError, match="SVD's AutoencoderKLTemporalDecoder is not covered"):
        P.AutoencoderKLDecoder(**TINY).load_state_dict(sd)


def test_save_pretrained_round_trip(tmp_path):
    import ctrl_adapter_amd as P
    ref = _seeded_tiny()
    m = P.AutoencoderKLDecoder(**TINY)
    m.load_state_dict(ref.state_dict())
    m.save_pretrained(str(tmp_path), safe_serialization=False)
    m2 = P.AutoencoderKLDecoder.from_pretrained(str(tmp_path))
    assert set(m2.state_dict()) == set(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    assert tuple(m2.config.block_out_channels) == tuple(TINY["block_out_channels"])


@pytest.mark.parametrize("kw,field", [
    (dict(out_channels=4), "out_channels"),
    (dict(up_block_types=("UpDecoderBlock2D", "AttnUpDecoderBlock2D")), "up_block_types"),
    (dict(norm_num_groups=16), "norm_num_groups"),
    (dict(block_out_channels=(48, 64)), "block_out_channels"),
    (dict(block_out_channels=(32, 4096)), "block_out_channels"),
    (dict(latent_channels=16), "latent_channels"),
    (dict(use_post_quant_conv=False), "use_post_quant_conv"),
    (dict(layers_per_block=9), "layers_per_block"),
    (dict(act_fn="relu"), "act_fn"),
    (dict(mid_block_add_attention=False), "mid_block_add_attention"),
])
def test_unsupported_configs_raise(kw, field):
    import ctrl_adapter_amd as P
    cfg = dict(TINY)
    cfg["up_block_types"] = ("UpDecoderBlock2D",) * len(kw.get("block_out_channels", cfg["block_out_channels"]))
    cfg.update(kw)
    with pytest.raises(ValueError, match=field):
        P.AutoencoderKLDecoder(**cfg)


@pytest.mark.parametrize("kw,field", [(dict(norm_num_groups=16), "norm_num_groups"), (dict(in_channels=4), "in_channels"),
                                      (dict(out_channels=4), "out_channels")])
def test_whole_vae_names_itself_in_config_errors(kw, field):
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError, match=r"^AutoencoderKL \(libctrlhip\): .*" + field):
        P.AutoencoderKL(**dict(TINY, **kw))


def test_config_struct_matches_header_and_abi_version():
    from ctrl_adapter_amd import _lib
    src = '#include "ctrl_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %d\\n", sizeof(ctrl_vae_decoder_config), CTRL_ABI_VERSION);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    assert [int(v) for v in out] == [ctypes.sizeof(_lib.VaeDecoderConfig), 11]
    assert _lib.VaeDecoderConfig.out_channels.offset == _lib.VaeDecoderConfig.norm_eps.offset + 4
    assert _lib.ABI_VERSION == 11 and _lib.lib().ctrl_abi_version() == 11
    assert (_lib.VAE_DEC_SAMPLE, _lib.VAE_DEC_UNIT, _lib.VAE_DEC_U8) == (0, 1, 2)


def test_new_symbols_resolve():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_vae_decoder_param_count", "ctrl_vae_decoder_param_spec", "ctrl_vae_decoder_create", "ctrl_vae_decoder_destroy",
                 "ctrl_vae_decoder_forward", "ctrl_vae_decoder_forward_strided", "ctrl_op_vae_dec_head", "ctrl_op_vae_dec_tail"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_restated_upsample_is_nearest_then_conv():
    g = torch.Generator().manual_seed(0)
    u = UpsampleRef(32)
    x = torch.randn(2, 32, 5, 7, generator=g)
    want = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), u.conv.weight, u.conv.bias, padding=1)
    got = u(x)
    assert got.shape == (2, 32, 10, 14)
    assert torch.equal(got, want)
    # nearest x2: output pixel (y, x) reads input pixel (y // 2, x // 2)
    up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    yy, xx = torch.arange(10) // 2, torch.arange(14) // 2
    assert torch.equal(up, x[:, :, yy][:, :, :, xx])


def test_u8_formula_with_ties():
    # x / 2 + 0.5 = k / 255 + half a level for the ties: (k + 0.5) / 255 * 255 rounds half to even in numpy
    ks = torch.arange(0, 255, dtype=torch.float64)
    ties = ((ks + 0.5) / 255.0 - 0.5) * 2.0
    x = torch.cat([ties.float(), torch.tensor([-3.0, -1.0, -0.999, 0.0, 0.999, 1.0, 3.0]), torch.linspace(-1.2, 1.2, 4001)])
    x = x.view(1, 1, 1, -1).expand(1, 3, 1, -1)
    want = (np.clip(x.permute(0, 2, 3, 1).numpy() / 2 + 0.5, 0, 1) * 255).round().astype("uint8")
    got = u8_of_sample(x)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    v = (x[0, 0, 0, :255].numpy() / 2 + 0.5) * 255                 # the ties that are exact in fp32 round half to EVEN, not up
    exact = v == np.floor(v) + 0.5
    assert exact.sum() >= 8
    assert (got[0, 0, :255, 0][exact] % 2 == 0).all() and (got[0, 0, :255, 0][exact] % 4 == 2).any()
    assert got.min() == 0 and got.max() == 255


def test_sdxl_helper_on_cpu_equals_restated_method():
    import ctrl_adapter_amd as P
    ref = _seeded_tiny().eval()
    lat = seeded_latents(2, 6, 5, seed=3) * ref.config.scaling_factor
    for ot in ("pt", "np"):
        with torch.no_grad():
            got, want = P.decode_sdxl_latents(ref, lat, ot), sdxl_decode_latents(ref, lat, ot)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(np.asarray(got), np.asarray(want))
    assert tuple(P.decode_sdxl_latents(ref, lat, "pt").shape) == (2, 3, 12, 10)
    assert P.decode_sdxl_latents(ref, lat, "np").shape == (2, 12, 10, 3)
    pil = P.decode_sdxl_latents(ref, lat, "pil")
    assert len(pil) == 2 and pil[0].size == (10, 12) and pil[0].mode == "RGB"
    with torch.no_grad():
        assert np.array_equal(pil_to_u8(pil), sdxl_decode_latents(ref, lat, "pil"))
    assert P.decode_sdxl_latents(ref, lat, "latent") is lat
    with pytest.raises(ValueError, match="output_type"):
        P.decode_sdxl_latents(ref, lat, "jpeg")


@pytest.mark.parametrize("chunk", [None, 4, 3])
def test_i2vgen_helper_on_cpu_equals_restated_method(chunk):
    import ctrl_adapter_amd as P
    ref = _seeded_tiny().eval()
    B, Fr = 2, 5                                                  # 10 frames: a chunk of 3 or 4 does not divide them
    lat = torch.randn(B, 4, Fr, 4, 6, generator=torch.Generator().manual_seed(5)) * ref.config.scaling_factor
    got = P.decode_i2vgen_latents(ref, lat, decode_chunk_size=chunk)
    with torch.no_grad():
        want = i2vgen_decode_latents(ref, lat, decode_chunk_size=chunk)
    assert got.shape == want.shape == (B, 3, Fr, 8, 12) and got.dtype == torch.float32
    assert torch.equal(got, want)
    # frame order: frame f of clip b is the decode of latents[b, :, f] alone
    with torch.no_grad():
        one = ref.decode(lat[1, :, 3].unsqueeze(0) / ref.config.scaling_factor).sample
    assert torch.allclose(got[1, :, 3], one[0], atol=1e-5)


def test_whole_vae_module_keys_and_config():
    import ctrl_adapter_amd as P
    with torch.device("meta"):
        ref = VaeRef(**SD_VAE)
    m = P.AutoencoderKL(**SD_VAE, force_upcast=True, scaling_factor=0.13025)
    assert _shapes(m.state_dict()) == _shapes(ref.state_dict())
    assert m.config.force_upcast is False and m.config["force_upcast"] is False
    assert m.config.scaling_factor == 0.13025 and m.config.latent_channels == 4 and len(m.config.block_out_channels) == 4
    assert m.dtype == torch.float32 and m.device.type == "cpu"
    assert isinstance(m, P.AutoencoderKLEncoder)                     # the encoder helpers take it as the mirror
    # a whole checkpoint loads, legacy attention names of both halves included, and round-trips through save_pretrained
    tiny = _seeded_tiny(VaeRef)
    sd = {}
    for k, v in tiny.state_dict().items():
        if ".attentions.0.to_q." in k:
            k = k.replace("to_q", "query")
        sd[k] = v
    t = P.AutoencoderKL(**TINY)
    t.load_state_dict(sd)
    for k, v in tiny.state_dict().items():
        assert torch.equal(t.state_dict()[k], v), k
    with tempfile.TemporaryDirectory() as d:
        t.save_pretrained(d)
        t2 = P.AutoencoderKL.from_pretrained(d, torch_dtype=torch.float16)
    assert t2.dtype == torch.float16 and t2.config.force_upcast is False
    assert set(t2.state_dict()) == set(tiny.state_dict())
    # the decoder alone loads the same whole checkpoint
    P.AutoencoderKLDecoder(**TINY).load_state_dict(tiny.state_dict())
    with pytest.raises(ValueError, match="up_block_types"):
        P.AutoencoderKL(**TINY, up_block_types=("UpDecoderBlock2D", "AttnUpDecoderBlock2D"))


def test_forward_without_gpu_raises():
    import ctrl_adapter_amd as P
    with pytest.raises(RuntimeError):
        P.AutoencoderKLDecoder(**TINY).decode(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError):
        P.AutoencoderKL(**TINY).decode(torch.zeros(1, 4, 4, 4))


def test_decoder_kernels_do_not_spill():
    """hipcc cross-compiles gfx950 here: the head kernel and the RGB tail kernel keep everything in registers (no VGPR spill, nothing in
    scratch); the tail's weights travel through scalar registers"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("igemm_resources", os.path.join(ROOT, "tools", "igemm_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    res = tool.analyse(os.path.join(ROOT, "ctrl-adapter_amd", "csrc", "vae.hip"))
    names = [n for n in res if "vae_dec_head_kernel" in n or ("vae_dec_tail_kernel" in n and "ILi3E" in n)]
    assert len(names) == 2, sorted(res)
    for n in names:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch"] == 0 and res[n]["sgpr_spill"] == 0, (n, res[n])
        assert res[n]["vgpr"] <= 128, (n, res[n])
