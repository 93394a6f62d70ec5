"""Temporal KL-VAE decoder, host side (no GPU): the parameter inventory against the restatement's diffusers keys
(tests/vae_tdecoder_ref.py), persistence, the pipeline-facing surface (forward's num_frames parameter, force_upcast), the refusals, the
restatement held bit for bit against the image decoder's restatement with the temporal branch switched off, and svd_decode_latents /
decode_svd_latents over chunks that straddle clips."""
import inspect

import pytest
import torch

from vae_decoder_ref import VaeDecoderRef, seeded_latents
from vae_tdecoder_ref import (MIX_CYCLE, SD_VAE, TINY, VaeTemporalDecoderRef, VaeTemporalRef, seeded_tdecoder, set_distinct_mix_factors,
                              svd_decode_latents)

# two mid ResNets around the attention, as the SVD VAE has (TINY's layers_per_block = 1 leaves the mid block one ResNet and an attention
# that diffusers' zip() never runs)
TINY2 = dict(block_out_channels=(32, 64), layers_per_block=2, latent_channels=4)


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("cfg", [SD_VAE, TINY, TINY2], ids=["sd_vae", "tiny", "tiny2"])
def test_param_spec_equals_diffusers_keys(cfg):
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.vae_temporal_decoder import vae_tdecoder_spec
    with torch.device("meta"):
        ref = VaeTemporalDecoderRef(**cfg)
        whole = VaeTemporalRef(**cfg)
    m = P.AutoencoderKLTemporalDecoder(**cfg)
    assert dict(vae_tdecoder_spec(m._dec_cfg)) == _shapes(ref.state_dict())
    assert _shapes(m.state_dict()) == _shapes(whole.state_dict())
    sd = _shapes(m.state_dict())
    assert not any(k.startswith("post_quant_conv") for k in sd)
    assert sd["decoder.time_conv_out.weight"] == (3, 3, 3, 1, 1)
    assert sd["decoder.mid_block.resnets.0.time_mixer.mix_factor"] == (1,)
    Ct = cfg["block_out_channels"][-1]
    assert sd["decoder.up_blocks.0.resnets.0.temporal_res_block.conv1.weight"] == (Ct, Ct, 3, 1, 1)
    assert ("decoder.mid_block.resnets.1.spatial_res_block.conv1.weight" in sd) == (cfg["layers_per_block"] >= 2)


def test_new_symbols_resolve_and_abi_version_stays():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in ("ctrl_vae_tdecoder_param_count", "ctrl_vae_tdecoder_param_spec", "ctrl_vae_tdecoder_create", "ctrl_vae_tdecoder_destroy",
                 "ctrl_vae_tdecoder_forward", "ctrl_op_vae_time_conv"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 11 and lib.ctrl_abi_version() == 11


def test_state_dict_and_save_pretrained_round_trip(tmp_path):
    import ctrl_adapter_amd as P
    ref = seeded_tdecoder(VaeTemporalRef, TINY, 11)
    m = P.AutoencoderKLTemporalDecoder(**TINY, scaling_factor=0.25)
    m.load_state_dict(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    mixes = [float(v) for k, v in m.state_dict().items() if k.endswith("mix_factor")]
    assert set(mixes) == set(MIX_CYCLE)                      # the values as loaded: the negation lives in the plan, not in the module
    m.save_pretrained(str(tmp_path))
    m2 = P.AutoencoderKLTemporalDecoder.from_pretrained(str(tmp_path), torch_dtype=torch.float16)
    assert m2.dtype == torch.float16 and m2.config.scaling_factor == 0.25
    assert tuple(m2.config.block_out_channels) == tuple(TINY["block_out_channels"]) and m2.config.force_upcast is False
    assert set(m2.state_dict()) == set(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k].float(), v), k


def test_pipeline_surface():
    import ctrl_adapter_amd as P
    m = P.AutoencoderKLTemporalDecoder(**TINY, force_upcast=True)
    assert "num_frames" in inspect.signature(m.forward).parameters          # what SVD's decode_latents inspects
    assert "num_frames" in inspect.signature(m.decode).parameters
    assert m.config.force_upcast is False and m.config["force_upcast"] is False
    assert m.config.latent_channels == 4 and m.config.scaling_factor == 0.18215
    assert m.dtype == torch.float32 and m.device.type == "cpu"
    assert isinstance(m, P.AutoencoderKLEncoder) and not isinstance(m, P.AutoencoderKL)
    assert m.up_factor == 2
    with pytest.raises(ValueError, match=r"^AutoencoderKLTemporalDecoder \(libctrlhip\): .*out_channels"):
        P.AutoencoderKLTemporalDecoder(**TINY, out_channels=4)


def test_refusals():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    from vae_decoder_ref import VaeRef
    plain = seeded_init(VaeRef(**TINY), seed=11).state_dict()
    with pytest.raises(ValueError, match="not a temporal-decoder checkpoint"):
        P.AutoencoderKLTemporalDecoder(**TINY).load_state_dict(plain)
    temporal = seeded_tdecoder(VaeTemporalRef, TINY, 11).state_dict()
    for cls in (P.AutoencoderKL, P.AutoencoderKLDecoder):
        with pytest.raises(ValueError, match="SVD's AutoencoderKLTemporalDecoder is not covered"):
            cls(**TINY).load_state_dict(temporal)
    m = P.AutoencoderKLTemporalDecoder(**TINY)
    with pytest.raises(ValueError, match="whole clips"):
        m.decode(torch.zeros(5, 4, 4, 4), num_frames=2)
    with pytest.raises(ValueError, match="frames_per_launch"):
        m.run_decoder(torch.zeros(4, 4, 4, 4), 2, frames_per_launch=0)
    with pytest.raises(RuntimeError):                                       # no CPU path
        m.decode(torch.zeros(4, 4, 4, 4), num_frames=2)


def _as_image_decoder(tref, cfg):
    """the image decoder's restatement with the temporal restatement's spatial weights and an identity post_quant_conv"""
    ref = VaeDecoderRef(**cfg)
    sd = {}
    for k, v in tref.state_dict().items():
        if ".temporal_res_block." in k or ".time_mixer." in k or ".time_conv_out." in k:
            continue
        sd[k.replace(".spatial_res_block.", ".")] = v
    lat = cfg["latent_channels"]
    sd["post_quant_conv.weight"] = torch.eye(lat).view(lat, lat, 1, 1)
    sd["post_quant_conv.bias"] = torch.zeros(lat)
    ref.load_state_dict(sd)
    return ref.eval()


@pytest.mark.parametrize("Fr", [1, 3])
def test_restatement_equals_image_decoder_with_the_temporal_branch_off(Fr):
    """mix_factor = -40: sigmoid is 4e-18, so 1 - sigmoid is exactly 1.0 in fp32 and the temporal branch's contribution rounds away;
    time_conv_out = the identity centre tap.  What is left is the image decoder, frame by frame, bit for bit."""
    from ctrl_adapter_amd.synthetic import seeded_init
    tref = seeded_init(VaeTemporalDecoderRef(**TINY2), seed=5).eval()
    with torch.no_grad():
        for k, p in tref.named_parameters():
            if k.endswith("mix_factor"):
                p.fill_(-40.0)
        assert float(1.0 - torch.sigmoid(torch.tensor([-40.0]))) == 1.0
        w = tref.decoder.time_conv_out.weight
        w.zero_()
        for c in range(w.shape[0]):
            w[c, c, 1, 0, 0] = 1.0
        tref.decoder.time_conv_out.bias.zero_()
        ref = _as_image_decoder(tref, TINY2)
        z = seeded_latents(Fr, 6, 5, seed=3)
        got = tref.decode(z, Fr).sample
        want = ref.decode(z).sample
    assert got.shape == want.shape == (Fr, 3, 12, 10)
    assert torch.equal(got, want)


def test_temporal_branch_and_mixers_matter():
    """the guard of the test above: with the seeded mixers the temporal branch moves the output, and another mixer order moves it too"""
    tref = seeded_tdecoder(VaeTemporalDecoderRef, TINY2, 5)
    z = seeded_latents(3, 6, 5, seed=3)
    with torch.no_grad():
        a = tref.decode(z, 3).sample
        one = tref.decode(z, 1).sample                      # the same frames as three one-frame clips
        for k, p in tref.named_parameters():
            if k.endswith("mix_factor"):
                p.neg_()
        b = tref.decode(z, 3).sample
    scale = a.abs().max()
    assert (a - one).abs().max() > 0.01 * scale and (a - b).abs().max() > 0.01 * scale
    vals = [float(p.detach()) for k, p in set_distinct_mix_factors(tref).named_parameters() if k.endswith("mix_factor")]
    assert vals[:4] == [MIX_CYCLE[0], MIX_CYCLE[1], MIX_CYCLE[2], MIX_CYCLE[0]]


def test_svd_decode_latents_chunks_straddle_clips():
    import ctrl_adapter_amd as P
    ref = seeded_tdecoder(VaeTemporalRef, TINY, 7)
    sf = ref.config.scaling_factor
    B, Fr = 2, 3
    lat = torch.randn(B, Fr, 4, 4, 6, generator=torch.Generator().manual_seed(5)) * sf
    with torch.no_grad():
        got = svd_decode_latents(ref, lat, Fr, decode_chunk_size=4)
        flat = 1 / sf * lat.flatten(0, 1)
        parts = [ref.decode(flat[0:4], 4).sample, ref.decode(flat[4:6], 2).sample]       # chunks of 4 (frame 3 is clip 1's first) and 2
        want = torch.cat(parts).reshape(B, Fr, 3, 8, 12).permute(0, 2, 1, 3, 4)
    assert got.shape == (B, 3, Fr, 8, 12) and got.dtype == torch.float32
    assert torch.equal(got, want)
    # the chunking is visible: a chunk is one clip, so frame 2 of clip 0 sees frame 0 of clip 1 behind it
    with torch.no_grad():
        whole = svd_decode_latents(ref, lat, Fr, decode_chunk_size=3)
    assert not torch.equal(got[0, :, 2], whole[0, :, 2])
    # the helper with a torch VAE takes the pipeline's route
    helper = P.decode_svd_latents(ref, lat, Fr, decode_chunk_size=4)
    assert helper.dtype == torch.float32 and torch.equal(helper, got)

    class NoFrames(torch.nn.Module):                       # a VAE whose forward has no num_frames parameter gets none
        config = ref.config

        def forward(self, sample):
            return sample

        def decode(self, z, **kw):
            assert kw == {}
            return ref.decode(z, z.shape[0])

    assert torch.equal(P.decode_svd_latents(NoFrames(), lat, Fr, decode_chunk_size=4), got)
