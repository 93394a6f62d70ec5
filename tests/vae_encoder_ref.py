"""fp32 PyTorch restatement of diffusers v0.27.2's KL-VAE encoder (Encoder + quant_conv + DiagonalGaussianDistribution, the encoder half
of AutoencoderKL and of SVD's AutoencoderKLTemporalDecoder) and of the two pipeline methods that call it (SVD's _encode_vae_image,
I2VGen-XL's prepare_image_latents).  Our own code, written from diffusers' semantics with plain F.conv2d / F.group_norm /
F.scaled_dot_product_attention; diffusers is not available here, so this restatement is NOT pinned against it.  Same keys
and encode() interface as ctrl_adapter_amd.AutoencoderKLEncoder."""
import torch
import torch.nn.functional as F
from torch import nn

# the SD-1.5 / SDXL / SVD VAE
SD_VAE = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4)
TINY = dict(block_out_channels=(32, 64), layers_per_block=1, latent_channels=4)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers.utils.torch_utils.randn_tensor for one generator (a CPU generator draws on the CPU, then moves)"""
    device = torch.device(device) if device is not None else torch.device("cpu")
    rand_device = device
    if generator is not None and generator.device.type != device.type and generator.device.type == "cpu":
        rand_device = torch.device("cpu")
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype).to(device)


class ResnetRef(nn.Module):
    """ResnetBlock2D without temb: x + conv2(SiLU(norm2(conv1(SiLU(norm1(x)))))), 1x1 conv_shortcut on x when the width changes"""

    def __init__(self, cin, cout, eps=1e-6):
        super().__init__()
        self.norm1 = nn.GroupNorm(32, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(32, cout, eps=eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return (self.conv_shortcut(x) if self.conv_shortcut is not None else x) + h


class DownsampleRef(nn.Module):
    """Downsample2D(use_conv=True, padding=0): F.pad(x, (0, 1, 0, 1)) then a stride-2 3x3 conv without padding"""

    def __init__(self, C):
        super().__init__()
        self.conv = nn.Conv2d(C, C, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0))


class AttentionRef(nn.Module):
    """the mid block's Attention: GroupNorm, ONE head of dim C (to_q / to_k / to_v / to_out.0 with bias), softmax in fp32, + residual"""

    def __init__(self, C, eps=1e-6):
        super().__init__()
        self.group_norm = nn.GroupNorm(32, C, eps=eps)
        self.to_q, self.to_k, self.to_v = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)
        self.to_out = nn.ModuleList([nn.Linear(C, C)])

    def forward(self, x):
        B, C, H, W = x.shape
        h = self.group_norm(x).view(B, C, H * W).transpose(1, 2)
        q, k, v = self.to_q(h), self.to_k(h), self.to_v(h)
        o = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
        o = self.to_out[0](o)
        return o.transpose(1, 2).reshape(B, C, H, W) + x


class _Block(nn.Module):
    pass


class DiagonalGaussianRef:
    def __init__(self, parameters):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        eps = randn_tensor(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        return self.mean + self.std * eps


class _Out(tuple):
    def __new__(cls, latent_dist):
        self = super().__new__(cls, (latent_dist,))
        self.latent_dist = latent_dist
        return self


class VaeEncoderRef(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, scaling_factor=0.18215, **unused):
        super().__init__()
        boc = tuple(block_out_channels)
        self.config = _Cfg(block_out_channels=boc, layers_per_block=layers_per_block, latent_channels=latent_channels,
                           scaling_factor=scaling_factor)
        enc = nn.Module()
        enc.conv_in = nn.Conv2d(3, boc[0], 3, padding=1)
        enc.down_blocks = nn.ModuleList()
        cin = boc[0]
        for i, cout in enumerate(boc):
            b = _Block()
            b.resnets = nn.ModuleList()
            for _ in range(layers_per_block):
                b.resnets.append(ResnetRef(cin, cout))
                cin = cout
            if i + 1 < len(boc):
                b.downsamplers = nn.ModuleList([DownsampleRef(cout)])
            enc.down_blocks.append(b)
        mid = _Block()
        mid.resnets = nn.ModuleList([ResnetRef(cin, cin), ResnetRef(cin, cin)])
        mid.attentions = nn.ModuleList([AttentionRef(cin)])
        enc.mid_block = mid
        enc.conv_norm_out = nn.GroupNorm(32, cin, eps=1e-6)
        enc.conv_out = nn.Conv2d(cin, 2 * latent_channels, 3, padding=1)
        self.encoder = enc
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    def moments(self, x):
        e = self.encoder
        h = e.conv_in(x)
        for b in e.down_blocks:
            for r in b.resnets:
                h = r(h)
            if hasattr(b, "downsamplers"):
                h = b.downsamplers[0](h)
        h = e.mid_block.resnets[0](h)
        h = e.mid_block.attentions[0](h)
        h = e.mid_block.resnets[1](h)
        h = e.conv_out(F.silu(e.conv_norm_out(h)))
        return self.quant_conv(h)

    def encode(self, x, return_dict=True):
        dist = DiagonalGaussianRef(self.moments(x))
        return _Out(dist) if return_dict else (dist,)


def seeded_pixels(N, H, W, seed=0, device="cpu"):
    """a smooth image in [-1, 1] plus noise (the VAE's input range)"""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    ph = torch.rand(N, 3, 1, 1, generator=g) * 6.28
    x = 0.6 * torch.sin(3 * xx + 2 * yy + ph) + 0.3 * torch.rand(N, 3, H, W, generator=g) - 0.15
    return x.clamp(-1, 1).to(device)


def svd_encode_vae_image(vae, image, device, num_videos_per_prompt, do_classifier_free_guidance):
    """the SVD pipeline's _encode_vae_image, restated"""
    image = image.to(device=device)
    image_latents = vae.encode(image).latent_dist.mode()
    if do_classifier_free_guidance:
        image_latents = torch.cat([torch.zeros_like(image_latents), image_latents])
    return image_latents.repeat(num_videos_per_prompt, 1, 1, 1)


def i2vgen_prepare_image_latents(vae, image, device, num_frames, num_videos_per_prompt, do_classifier_free_guidance, generator=None):
    """I2VGen-XL's prepare_image_latents, restated (sample with an explicit generator)"""
    image = image.to(device=device)
    image_latents = vae.encode(image).latent_dist.sample(generator) * vae.config.scaling_factor
    image_latents = image_latents.unsqueeze(2)
    mask = [torch.ones_like(image_latents[:, :, :1]) * ((i + 1) / (num_frames - 1)) for i in range(num_frames - 1)]
    if mask:
        image_latents = torch.cat([image_latents, torch.cat(mask, dim=2)], dim=2)
    image_latents = image_latents.repeat(num_videos_per_prompt, 1, 1, 1, 1)
    if do_classifier_free_guidance:
        image_latents = torch.cat([image_latents] * 2)
    return image_latents
