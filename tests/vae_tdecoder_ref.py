"""fp32 PyTorch restatement of diffusers v0.27.2's temporal KL-VAE decoder (TemporalDecoder, AutoencoderKLTemporalDecoder.decode) and of
the SVD pipeline's decode_latents.  Our own code, written from diffusers' semantics with plain F.conv2d / F.conv3d / F.group_norm;
diffusers is not available here, so this restatement is NOT pinned against it -- tests/test_vae_tdecoder_host.py holds it
against the image decoder's restatement instead, bit for bit, with the temporal branch switched off.  The spatial ResNet, the attention
and the up-sampler are the other restatements' (tests/vae_encoder_ref.py, tests/vae_decoder_ref.py).  Same keys and decode() interface
as ctrl_adapter_amd.AutoencoderKLTemporalDecoder; VaeTemporalRef carries the whole VAE's keys."""
import inspect

import torch
import torch.nn.functional as F
from torch import nn

from vae_decoder_ref import UpsampleRef, _Sample
from vae_encoder_ref import SD_VAE, TINY, AttentionRef, ResnetRef, VaeEncoderRef, _Block, _Cfg  # noqa: F401

MIX_CYCLE = (-1.5, 0.5, 2.0)


class TemporalResnetRef(nn.Module):
    """TemporalResnetBlock(C, C) without temb on [B, C, F, H, W]: GroupNorm over the clip's (C / 32, F, H, W), SiLU, Conv3d (3,1,1)
    padding (1,0,0), the same again, + input"""

    def __init__(self, C, eps=1e-5):
        super().__init__()
        self.norm1 = nn.GroupNorm(32, C, eps=eps)
        self.conv1 = nn.Conv3d(C, C, (3, 1, 1), padding=(1, 0, 0))
        self.norm2 = nn.GroupNorm(32, C, eps=eps)
        self.conv2 = nn.Conv3d(C, C, (3, 1, 1), padding=(1, 0, 0))

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return x + h


class _Mixer(nn.Module):
    def __init__(self):
        super().__init__()
        self.mix_factor = nn.Parameter(torch.tensor([0.5]))


class SpatioTemporalResRef(nn.Module):
    """SpatioTemporalResBlock (merge strategy learned, switch_spatial_to_temporal_mix, no temb) on [B * F, C, H, W]:
    x_s = spatial(x); x_t = temporal(x_s as [B, C, F, H, W]); (1 - a) x_s + a x_t with a = sigmoid(mix_factor)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.spatial_res_block = ResnetRef(cin, cout, eps=1e-6)
        self.temporal_res_block = TemporalResnetRef(cout, eps=1e-5)
        self.time_mixer = _Mixer()

    def forward(self, x, num_frames):
        xs = self.spatial_res_block(x)
        BF, C, H, W = xs.shape
        x5 = xs.reshape(BF // num_frames, num_frames, C, H, W).permute(0, 2, 1, 3, 4)
        xt = self.temporal_res_block(x5)
        a = torch.sigmoid(self.time_mixer.mix_factor)
        y = (1.0 - a) * x5 + a * xt
        return y.permute(0, 2, 1, 3, 4).reshape(BF, C, H, W)


def _tdecoder_tree(boc, layers_per_block, latent_channels, out_channels=3):
    dec = nn.Module()
    rev = tuple(reversed(boc))
    dec.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
    mid = _Block()
    mid.resnets = nn.ModuleList([SpatioTemporalResRef(rev[0], rev[0]) for _ in range(layers_per_block)])
    mid.attentions = nn.ModuleList([AttentionRef(rev[0])])       # ONE attention whatever num_layers is: zip() below stops after it
    dec.mid_block = mid
    dec.up_blocks = nn.ModuleList()
    cin = rev[0]
    for i, cout in enumerate(rev):
        b = _Block()
        b.resnets = nn.ModuleList()
        for _ in range(layers_per_block + 1):
            b.resnets.append(SpatioTemporalResRef(cin, cout))
            cin = cout
        if i + 1 < len(rev):
            b.upsamplers = nn.ModuleList([UpsampleRef(cout)])
        dec.up_blocks.append(b)
    dec.conv_norm_out = nn.GroupNorm(32, cin, eps=1e-6)
    dec.conv_out = nn.Conv2d(cin, out_channels, 3, padding=1)
    dec.time_conv_out = nn.Conv3d(out_channels, out_channels, (3, 1, 1), padding=(1, 0, 0))
    return dec


def _tdecode(m, z, num_frames):
    d = m.decoder
    h = d.conv_in(z)
    h = d.mid_block.resnets[0](h, num_frames)
    for r, attn in zip(d.mid_block.resnets[1:], d.mid_block.attentions):
        h = attn(h)
        h = r(h, num_frames)
    for b in d.up_blocks:
        for r in b.resnets:
            h = r(h, num_frames)
        if hasattr(b, "upsamplers"):
            h = b.upsamplers[0](h)
    h = d.conv_out(F.silu(d.conv_norm_out(h)))
    BF, C, H, W = h.shape
    h = h.reshape(BF // num_frames, num_frames, C, H, W).permute(0, 2, 1, 3, 4)
    h = d.time_conv_out(h)
    return h.permute(0, 2, 1, 3, 4).reshape(BF, C, H, W)


class VaeTemporalDecoderRef(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, scaling_factor=0.18215,
                 force_upcast=True, **unused):
        super().__init__()
        boc = tuple(block_out_channels)
        self.config = _Cfg(block_out_channels=boc, layers_per_block=layers_per_block, latent_channels=latent_channels,
                           scaling_factor=scaling_factor, force_upcast=force_upcast)
        self.decoder = _tdecoder_tree(boc, layers_per_block, latent_channels)

    @property
    def dtype(self):
        return self.decoder.conv_in.weight.dtype

    def decode(self, z, num_frames, return_dict=True):
        s = _tdecode(self, z, num_frames)
        return _Sample(s) if return_dict else (s,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None, num_frames=1):
        raise NotImplementedError("the decoder restatement has no encoder")


class VaeTemporalRef(VaeEncoderRef):
    """the whole AutoencoderKLTemporalDecoder: the encoder restatement (encoder.*, quant_conv.*) plus the temporal decoder"""

    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, scaling_factor=0.18215,
                 force_upcast=True, **unused):
        super().__init__(block_out_channels=block_out_channels, layers_per_block=layers_per_block, latent_channels=latent_channels,
                         scaling_factor=scaling_factor)
        self.config["force_upcast"] = force_upcast
        self.decoder = _tdecoder_tree(tuple(block_out_channels), layers_per_block, latent_channels)

    @property
    def dtype(self):
        return self.quant_conv.weight.dtype

    def decode(self, z, num_frames, return_dict=True):
        s = _tdecode(self, z, num_frames)
        return _Sample(s) if return_dict else (s,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None, num_frames=1):
        dist = self.encode(sample).latent_dist
        z = dist.sample(generator=generator) if sample_posterior else dist.mode()
        return self.decode(z, num_frames=num_frames, return_dict=return_dict)


@torch.no_grad()
def set_distinct_mix_factors(module):
    """after seeded_init (which sets every mix_factor to 0.5): distinct values cycling through -1.5, 0.5 and 2.0 in state-dict order, so
    that a swapped blend (sigmoid for 1 - sigmoid) or a mixer read from another block is an O(0.1) error"""
    i = 0
    for name, p in module.named_parameters():
        if name.endswith("mix_factor"):
            p.fill_(MIX_CYCLE[i % len(MIX_CYCLE)])
            i += 1
    assert i > 0
    return module


def seeded_tdecoder(cls, cfg, seed):
    """cls(**cfg) with synthetic.seeded_init weights and distinct mix factors"""
    from ctrl_adapter_amd.synthetic import seeded_init
    return set_distinct_mix_factors(seeded_init(cls(**cfg), seed=seed)).eval()


def svd_decode_latents(vae, latents, num_frames, decode_chunk_size=14):
    """the SVD pipeline's decode_latents, restated"""
    latents = latents.flatten(0, 1)
    latents = 1 / vae.config.scaling_factor * latents
    accepts_num_frames = "num_frames" in set(inspect.signature(vae.forward).parameters.keys())
    frames = []
    for i in range(0, latents.shape[0], decode_chunk_size):
        num_frames_in = latents[i:i + decode_chunk_size].shape[0]
        kw = {"num_frames": num_frames_in} if accepts_num_frames else {}
        frames.append(vae.decode(latents[i:i + decode_chunk_size], **kw).sample)
    frames = torch.cat(frames, dim=0)
    frames = frames.reshape(-1, num_frames, *frames.shape[1:]).permute(0, 2, 1, 3, 4)
    return frames.float()
