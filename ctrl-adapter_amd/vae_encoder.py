"""AutoencoderKLEncoder -- the encoder half of diffusers' AutoencoderKL / AutoencoderKLTemporalDecoder (Encoder + quant_conv +
DiagonalGaussianDistribution, diffusers v0.27) whose forward runs in libctrlhip (csrc/vae.hip, csrc/plan_vae.cpp), and the two video
pipelines' image-latent steps:

  encode_svd_image_latents      svd/pipelines/svd_controlnet_adapter_pipeline.py:214-235 (_encode_vae_image: latent_dist.mode())
  prepare_i2vgen_image_latents  i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:487-518 (prepare_image_latents:
                                latent_dist.sample() * scaling_factor + the frame-position mask)

State-dict keys are diffusers' (`encoder.conv_in.weight`, ..., `quant_conv.bias`); a full VAE checkpoint loads (decoder.* and
post_quant_conv.* are ignored), and so do the legacy attention names (query / key / value / proj_attn)."""
import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec

_LEGACY_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def _vae_config(block_out_channels, layers_per_block, latent_channels, norm_num_groups, out_channels=None):
    """the encoder's ctrl_vae_encoder_config, or with out_channels the decoder's ctrl_vae_decoder_config"""
    cfg = L.VaeEncoderConfig() if out_channels is None else L.VaeDecoderConfig()
    cfg.num_levels = len(block_out_channels)
    for i, c in enumerate(block_out_channels):
        cfg.block_out_channels[i] = int(c)
    cfg.layers_per_block, cfg.latent_channels, cfg.norm_num_groups = layers_per_block, latent_channels, norm_num_groups
    cfg.norm_eps = 1e-6
    if out_channels is not None:
        cfg.out_channels = out_channels
    return cfg


_HALF_NAMES = {"encoder": ("in_channels", "down_block_types", "DownEncoderBlock2D", "use_quant_conv"),
               "decoder": ("out_channels", "up_block_types", "UpDecoderBlock2D", "use_post_quant_conv")}


def _check_vae_config(who, half, io_channels, block_types, block_out_channels, layers_per_block, act_fn, latent_channels,
                      norm_num_groups, use_conv, mid_block_add_attention):
    """what the plan of one half ("encoder" | "decoder") of a KL-VAE covers, refused in the name of the class `who`; io_channels,
    block_types and use_conv are the half's in / out channels, down / up block types and use_quant_conv / use_post_quant_conv"""
    pre = "%s (libctrlhip): " % who
    io_name, types_name, block, conv_name = _HALF_NAMES[half]
    if io_channels != 3:
        raise ValueError(pre + "%s must be 3 (got %r)" % (io_name, io_channels))
    if not 1 <= len(block_out_channels) <= 4:
        raise ValueError(pre + "block_out_channels must hold 1 to 4 values")
    if tuple(block_types) != (block,) * len(block_out_channels):
        raise ValueError(pre + "%s must all be %s, one per block_out_channels entry (got %r)" % (types_name, block, tuple(block_types)))
    if norm_num_groups != 32:
        raise ValueError(pre + "norm_num_groups must be 32 (got %r)" % (norm_num_groups,))
    if any(c % 32 or not 32 <= c <= 2048 for c in block_out_channels):
        raise ValueError(pre + "block_out_channels must be multiples of 32 up to 2048 (got %r)" % (block_out_channels,))
    if not 1 <= latent_channels <= 8:
        raise ValueError(pre + "latent_channels must be 1 .. 8 (got %r)" % (latent_channels,))
    if not use_conv:
        raise ValueError(pre + "%s must be True" % conv_name)
    if not 1 <= layers_per_block <= 8:
        raise ValueError(pre + "layers_per_block must be 1 .. 8 (got %r)" % (layers_per_block,))
    if act_fn != "silu":
        raise ValueError(pre + "act_fn must be silu (got %r)" % (act_fn,))
    if not mid_block_add_attention:
        raise ValueError(pre + "mid_block_add_attention must be True")


def _map_vae_keys(state_dict, drop, halves=("decoder",)):
    """diffusers' keys out of a VAE state dict: keys under the `drop` prefixes left out, the legacy attention names of the mid blocks of
    `halves` (encoder / decoder) mapped to to_q / to_k / to_v / to_out.0 (a 1 x 1 conv weight of the oldest checkpoints squeezed to the
    linear's [C][C]); with the decoder among `halves` a temporal-decoder checkpoint is refused"""
    sd = {}
    legacy = tuple(half + ".mid_block.attentions." for half in halves)
    for key, v in state_dict.items():
        if "decoder" in halves and key.startswith("decoder.up_blocks.") and ".spatial_res_block." in key:
            raise ValueError("this is a temporal-decoder checkpoint (%s): SVD's AutoencoderKLTemporalDecoder is not covered by the "
                             "libctrlhip KL-VAE decoder" % key)
        if drop and key.startswith(drop):
            continue
        parts = key.split(".")
        if key.startswith(legacy) and len(parts) >= 6 and parts[4] in _LEGACY_ATTN:
            key = ".".join(parts[:4] + [_LEGACY_ATTN[parts[4]]] + parts[5:])
            if v.dim() == 4 and v.shape[2:] == (1, 1):
                v = v[:, :, 0, 0]
        sd[key] = v
    return sd


def vae_encoder_spec(cfg):
    """(name, shape) of every parameter of a ctrl_vae_encoder_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_vae_encoder_param_count, lib.ctrl_vae_encoder_param_spec, cfg)


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers.utils.torch_utils.randn_tensor: the same generator gives the same noise (a CPU generator draws on the CPU)"""
    device = torch.device(device) if device is not None else torch.device("cpu")
    rand_device = device
    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if generator is not None:
        gen_type = generator[0].device.type if isinstance(generator, list) else generator.device.type
        if gen_type != device.type and gen_type == "cpu":
            rand_device = torch.device("cpu")
        elif gen_type != device.type and gen_type == "cuda":
            raise ValueError("Cannot generate a %s tensor from a generator of type %s." % (device, gen_type))
    if isinstance(generator, list):
        one = (1,) + tuple(shape[1:])
        return torch.cat([torch.randn(one, generator=g, device=rand_device, dtype=dtype) for g in generator[:shape[0]]]).to(device)
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype).to(device)


def _posterior(moments, lat, kind, eps=None, scale=1.0, out_dtype=torch.float32):
    """ctrl_op_vae_posterior on MOMENTS planes [N][4*lat][h][w] fp32 (mean | logvar | std | var): mode / sample in out_dtype"""
    N, _, h, w = moments.shape
    out = torch.empty((N, lat, h, w), dtype=out_dtype, device=moments.device)
    e = eps.contiguous() if eps is not None else None
    with torch.cuda.device(moments.device):
        L.check(L.lib().ctrl_op_vae_posterior(L.ptr(moments), 4 * lat, 1, None, None, N, lat, h, w, L.ptr(e),
                                              L.dtype_code(e.dtype) if e is not None else 0, float(scale), kind, L.ptr(out),
                                              L.dtype_code(out_dtype), L.cur_stream()))
    return out


class DiagonalGaussianDistribution:
    """diffusers' DiagonalGaussianDistribution over the encoder's moments: mean / logvar (clamped to [-30, 20]) / std / var in the
    module's dtype, mode(), and sample(generator) whose noise is drawn as diffusers draws it and combined by the posterior kernel"""

    def __init__(self, moments, lat, dtype):
        self._moments, self._lat, self._dtype = moments, lat, dtype      # fp32 [N][4*lat][h][w]
        m = moments.to(dtype)
        self.mean, self.logvar, self.std, self.var = m[:, :lat], m[:, lat:2 * lat], m[:, 2 * lat:3 * lat], m[:, 3 * lat:]
        self.deterministic = False

    @property
    def parameters(self):
        return torch.cat([self.mean, self.logvar], dim=1)

    def mode(self):
        return self.mean

    def sample(self, generator=None, eps=None):
        if eps is None:
            eps = randn_tensor(self.mean.shape, generator=generator, device=self._moments.device, dtype=self._dtype)
        return _posterior(self._moments, self._lat, L.VAE_SAMPLE, eps=eps, out_dtype=self._dtype)


class AutoencoderKLOutput(tuple):
    """(latent_dist,) with attribute access, as diffusers' AutoencoderKLOutput"""

    def __new__(cls, latent_dist):
        self = super().__new__(cls, (latent_dist,))
        self.latent_dist = latent_dist
        return self


class AutoencoderKLEncoder(ParamTreeModule):
    """The encoder of diffusers' AutoencoderKL / AutoencoderKLTemporalDecoder (their config kwargs; the decoders are vae_decoder.py's and
    vae_temporal_decoder.py's).  An
    image's latents are bit-identical alone or inside any batch."""

    _CREATE, _DESTROY = "ctrl_vae_encoder_create", "ctrl_vae_encoder_destroy"
    _WHO = "AutoencoderKLEncoder"        # the class a refused configuration is reported for

    def __init__(self, in_channels=3, out_channels=3, down_block_types=None, up_block_types=None,
                 block_out_channels=(128, 256, 512, 512), layers_per_block=2, act_fn="silu", latent_channels=4, norm_num_groups=32,
                 sample_size=512, scaling_factor=0.18215, shift_factor=None, latents_mean=None, latents_std=None, force_upcast=True,
                 use_quant_conv=True, use_post_quant_conv=True, mid_block_add_attention=True, **unused):
        super().__init__()
        block_out_channels = tuple(int(c) for c in block_out_channels)
        if down_block_types is None:
            down_block_types = ("DownEncoderBlock2D",) * len(block_out_channels)
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__", "unused")})
        _check_vae_config(self._WHO, "encoder", in_channels, down_block_types, block_out_channels, layers_per_block, act_fn,
                          latent_channels, norm_num_groups, use_quant_conv, mid_block_add_attention)
        self._cfg = _vae_config(block_out_channels, layers_per_block, latent_channels, norm_num_groups)
        self.latent_channels = latent_channels
        self.down_factor = 2 ** (len(block_out_channels) - 1)
        self._register_spec(vae_encoder_spec(self._cfg), dtype=torch.float32)

    def config_dict(self):
        return dict(self.config)

    def load_state_dict(self, state_dict, strict=True, **k):
        """diffusers' keys of a whole VAE (decoder.* / post_quant_conv.* dropped), legacy attention names mapped to to_q / to_k / to_v /
        to_out.0 (a 1 x 1 conv weight of the oldest checkpoints squeezed to the linear's [C][C])"""
        return super().load_state_dict(_map_vae_keys(state_dict, ("decoder.", "post_quant_conv."), ("encoder",)), strict=strict, **k)

    def run(self, x, kind=L.VAE_MODE, eps=None, scale=1.0, out_dtype=None):
        """one ctrl_vae_encoder_forward: x [N, 3, H, W] fp32 / fp16 / bf16 on the GPU -> [N, lat, H/f, W/f] (mode: mean * scale;
        sample: (mean + std * eps) * scale) or [N, 4 * lat, H/f, W/f] (moments: mean | logvar | std | var) in out_dtype (default: the
        module's dtype)"""
        dev = _check_gpu_input(self, x, "the image")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("the image must be [N, 3, H, W] (got %s)" % (tuple(x.shape),))
        N, _, H, W = x.shape
        f, lat = self.down_factor, self.latent_channels
        if H % 8 or W % 8 or H % f or W % f:
            raise ValueError("H and W must be multiples of 8 and of %d (got %d x %d)" % (f, H, W))
        dt = self.dtype if out_dtype is None else out_dtype
        ch = 4 * lat if kind == L.VAE_MOMENTS else lat
        out = torch.empty((N, ch, H // f, W // f), dtype=dt, device=dev)
        e = None
        if kind == L.VAE_SAMPLE:
            if eps is None or tuple(eps.shape) != (N, lat, H // f, W // f) or eps.device != dev:
                raise ValueError("sampling needs eps [N, %d, %d, %d] on %s" % (lat, H // f, W // f, dev))
            e = eps.contiguous()
        if N == 0:
            return out
        px = x.contiguous()
        with torch.cuda.device(dev):
            plan = self._ensure_plan()
            L.check(L.lib().ctrl_vae_encoder_forward(plan, L.ptr(px), L.dtype_code(px.dtype), N, H, W, L.ptr(e),
                                                     L.dtype_code(e.dtype) if e is not None else 0, float(scale), int(kind), L.ptr(out),
                                                     L.dtype_code(dt), L.cur_stream()))
        L.raise_if_out_of_range("AutoencoderKLEncoder")
        return out

    def encode(self, x, return_dict=True):
        dist = DiagonalGaussianDistribution(self.run(x, L.VAE_MOMENTS, out_dtype=torch.float32), self.latent_channels, self.dtype)
        return AutoencoderKLOutput(dist) if return_dict else (dist,)

    def forward(self, x, return_dict=True):
        return self.encode(x, return_dict=return_dict)


def _is_mirror(vae):
    return isinstance(vae, AutoencoderKLEncoder)


def _scaling_factor(vae):
    cfg = vae.config
    return cfg["scaling_factor"] if isinstance(cfg, dict) else cfg.scaling_factor


@torch.no_grad()
def encode_svd_image_latents(vae, image, device, num_videos_per_prompt, do_classifier_free_guidance):
    """The SVD pipeline's _encode_vae_image (svd/pipelines/svd_controlnet_adapter_pipeline.py:214-235) with the VAE passed in:
    latent_dist.mode(), zero negatives first under CFG, then repeat(num_videos_per_prompt, 1, 1, 1).  On the mirror the mode leaves
    the posterior kernel directly."""
    image = image.to(device=device)
    if _is_mirror(vae):
        image_latents = vae.run(image, L.VAE_MODE)
    else:
        image_latents = vae.encode(image).latent_dist.mode()
    if do_classifier_free_guidance:
        image_latents = torch.cat([torch.zeros_like(image_latents), image_latents])
    return image_latents.repeat(num_videos_per_prompt, 1, 1, 1)


@torch.no_grad()
def prepare_i2vgen_image_latents(vae, image, device, num_frames, num_videos_per_prompt, do_classifier_free_guidance, generator=None):
    """The I2VGen-XL pipeline's prepare_image_latents (i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:487-518) with the
    VAE and the guidance flag passed in: latent_dist.sample(generator) * scaling_factor, the frame axis with the position mask
    (frame_idx + 1) / (num_frames - 1) on frames 1 .. F - 1 -> [B, lat, F, h, w], repeat per video, duplicated under CFG.  On the mirror
    the noise is drawn as diffusers draws it and the posterior kernel forms (mean + std * eps) * scaling_factor in fp32."""
    image = image.to(device=device)
    sf = _scaling_factor(vae)
    if _is_mirror(vae):
        N, _, H, W = image.shape
        f = vae.down_factor
        eps = randn_tensor((N, vae.latent_channels, H // f, W // f), generator=generator, device=image.device, dtype=vae.dtype)
        image_latents = vae.run(image, L.VAE_SAMPLE, eps=eps, scale=sf)
    else:
        image_latents = vae.encode(image).latent_dist.sample(generator) * sf
    image_latents = image_latents.unsqueeze(2)
    frame_position_mask = []
    for frame_idx in range(num_frames - 1):
        scale = (frame_idx + 1) / (num_frames - 1)
        frame_position_mask.append(torch.ones_like(image_latents[:, :, :1]) * scale)
    if frame_position_mask:
        image_latents = torch.cat([image_latents, torch.cat(frame_position_mask, dim=2)], dim=2)
    image_latents = image_latents.repeat(num_videos_per_prompt, 1, 1, 1, 1)
    if do_classifier_free_guidance:
        image_latents = torch.cat([image_latents] * 2)
    return image_latents
