"""fp32 PyTorch restatement of diffusers v0.27.2's KL-VAE decoder (post_quant_conv + Decoder, AutoencoderKL.decode) and of the two
pipeline methods that call it (the SDXL pipeline's final decode + VaeImageProcessor.postprocess, I2VGen-XL's decode_latents).  Our own
code, written from diffusers' semantics with plain F.conv2d / F.group_norm / F.interpolate; diffusers is not available here, so this
restatement is NOT pinned against it.  ResNet and attention are the encoder restatement's (tests/vae_encoder_ref.py).  Same
keys and decode() interface as ctrl_adapter_amd.AutoencoderKLDecoder; VaeRef carries the whole VAE's keys, as ctrl_adapter_amd.AutoencoderKL."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from vae_encoder_ref import SD_VAE, TINY, AttentionRef, ResnetRef, VaeEncoderRef, _Block, _Cfg  # noqa: F401


class UpsampleRef(nn.Module):
    """Upsample2D(use_conv=True): nearest x2, then a 3x3 conv of the same width"""

    def __init__(self, C):
        super().__init__()
        self.conv = nn.Conv2d(C, C, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class _Sample(tuple):
    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


def _decoder_tree(boc, layers_per_block, latent_channels, out_channels=3):
    dec = nn.Module()
    rev = tuple(reversed(boc))
    dec.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
    mid = _Block()
    mid.resnets = nn.ModuleList([ResnetRef(rev[0], rev[0]), ResnetRef(rev[0], rev[0])])
    mid.attentions = nn.ModuleList([AttentionRef(rev[0])])
    dec.mid_block = mid
    dec.up_blocks = nn.ModuleList()
    cin = rev[0]
    for i, cout in enumerate(rev):
        b = _Block()
        b.resnets = nn.ModuleList()
        for _ in range(layers_per_block + 1):
            b.resnets.append(ResnetRef(cin, cout))
            cin = cout
        if i + 1 < len(rev):
            b.upsamplers = nn.ModuleList([UpsampleRef(cout)])
        dec.up_blocks.append(b)
    dec.conv_norm_out = nn.GroupNorm(32, cin, eps=1e-6)
    dec.conv_out = nn.Conv2d(cin, out_channels, 3, padding=1)
    return dec


def _decode(m, z):
    d = m.decoder
    h = d.conv_in(m.post_quant_conv(z))
    h = d.mid_block.resnets[0](h)
    h = d.mid_block.attentions[0](h)
    h = d.mid_block.resnets[1](h)
    for b in d.up_blocks:
        for r in b.resnets:
            h = r(h)
        if hasattr(b, "upsamplers"):
            h = b.upsamplers[0](h)
    return d.conv_out(F.silu(d.conv_norm_out(h)))


class VaeDecoderRef(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, scaling_factor=0.18215,
                 force_upcast=True, **unused):
        super().__init__()
        boc = tuple(block_out_channels)
        self.config = _Cfg(block_out_channels=boc, layers_per_block=layers_per_block, latent_channels=latent_channels,
                           scaling_factor=scaling_factor, force_upcast=force_upcast)
        self.decoder = _decoder_tree(boc, layers_per_block, latent_channels)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)

    @property
    def dtype(self):
        return self.post_quant_conv.weight.dtype

    def decode(self, z, return_dict=True, generator=None):
        s = _decode(self, z)
        return _Sample(s) if return_dict else (s,)


class VaeRef(VaeEncoderRef):
    """the whole AutoencoderKL: the encoder restatement plus the decoder, the state-dict keys of a VAE checkpoint"""

    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, scaling_factor=0.18215,
                 force_upcast=True, **unused):
        super().__init__(block_out_channels=block_out_channels, layers_per_block=layers_per_block, latent_channels=latent_channels,
                         scaling_factor=scaling_factor)
        self.config["force_upcast"] = force_upcast
        self.decoder = _decoder_tree(tuple(block_out_channels), layers_per_block, latent_channels)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)

    @property
    def dtype(self):
        return self.post_quant_conv.weight.dtype

    def decode(self, z, return_dict=True, generator=None):
        s = _decode(self, z)
        return _Sample(s) if return_dict else (s,)


def seeded_latents(N, h, w, seed=0, device="cpu", lat=4):
    """N(0, 1) latents from a CPU generator (what the decoder sees after latents / scaling_factor, to first order)"""
    return torch.randn(N, lat, h, w, generator=torch.Generator().manual_seed(seed)).to(device)


def u8_of_sample(x):
    """numpy_to_pil's array of VaeImageProcessor.postprocess: denormalize, NHWC float32 numpy, (images * 255).round() as uint8"""
    img = (x / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
    return (img * 255).round().astype("uint8")


def sdxl_decode_latents(vae, latents, output_type="pil"):
    """the SDXL pipeline's final decode + VaeImageProcessor.postprocess, restated (no watermark); "pil" returns the uint8 NHWC array
    numpy_to_pil wraps, one PIL image per row"""
    needs_upcasting = vae.dtype == torch.float16 and vae.config.force_upcast
    if needs_upcasting:
        vae.to(dtype=torch.float32)
        latents = latents.to(torch.float32)
    image = vae.decode(latents / vae.config.scaling_factor, return_dict=False)[0]
    if needs_upcasting:
        vae.to(dtype=torch.float16)
    if output_type == "pil":
        return u8_of_sample(image)
    image = (image / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return image
    assert output_type == "np", output_type
    return image.cpu().permute(0, 2, 3, 1).float().numpy()


def i2vgen_decode_latents(vae, latents, decode_chunk_size=None):
    """I2VGen-XL's decode_latents, restated"""
    latents = 1 / vae.config.scaling_factor * latents
    B, C, Fr, h, w = latents.shape
    latents = latents.permute(0, 2, 1, 3, 4).reshape(B * Fr, C, h, w)
    if decode_chunk_size is not None:
        image = torch.cat([vae.decode(latents[i:i + decode_chunk_size]).sample for i in range(0, latents.shape[0], decode_chunk_size)], dim=0)
    else:
        image = vae.decode(latents).sample
    video = image[None, :].reshape((B, Fr, -1) + image.shape[2:]).permute(0, 2, 1, 3, 4)
    return video.float()


def pil_to_u8(images):
    """the uint8 NHWC array of a list of PIL images"""
    return np.stack([np.asarray(im) for im in images])
