"""AutoencoderKLDecoder -- the decoder half of diffusers' AutoencoderKL (post_quant_conv + Decoder, diffusers v0.27) whose forward runs
in libctrlhip (csrc/vae.hip, csrc/plan_vae_decoder.cpp); AutoencoderKL -- the whole VAE (this decoder and the encoder of vae_encoder.py
over one set of parameters), a drop-in for `pipe.vae`; and the two pipelines' decode steps:

  decode_sdxl_latents    sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1406-1427 (vae.decode(latents / scaling_factor) +
                         VaeImageProcessor.postprocess, without the watermark)
  decode_i2vgen_latents  i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:398-418 (decode_latents: frames in chunks,
                         [B, C, F, h, w] -> [B, 3, F, H, W] float32)

State-dict keys are diffusers' (`post_quant_conv.weight`, `decoder.conv_in.weight`, ...); a full VAE checkpoint loads into the decoder
(encoder.* and quant_conv.* are ignored), and so do the legacy attention names (query / key / value / proj_attn).  SVD's
AutoencoderKLTemporalDecoder is vae_temporal_decoder.py's: these classes refuse its checkpoint."""
import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec
from .vae_encoder import AutoencoderKLEncoder, _check_vae_config, _map_vae_keys, _scaling_factor, _vae_config

_KINDS = (L.VAE_DEC_SAMPLE, L.VAE_DEC_UNIT, L.VAE_DEC_U8)


def vae_decoder_spec(cfg):
    """(name, shape) of every parameter of a ctrl_vae_decoder_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_vae_decoder_param_count, lib.ctrl_vae_decoder_param_spec, cfg)


class DecoderOutput(tuple):
    """(sample,) with attribute access, as diffusers' DecoderOutput"""

    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


def _decoder_io(m, z, kind, out_dtype, out):
    """what every decoder forward of the module `m` (its device, dtype, latent_channels, up_factor) checks and prepares: (device, the
    latents as the head kernel can read them, the output tensor of `kind`, the dtype `sample` is rounded to)"""
    dev = _check_gpu_input(m, z, "the latents", "live")
    if z.dim() != 4 or z.shape[1] != m.latent_channels:
        raise ValueError("the latents must be [N, %d, h, w] (got %s)" % (m.latent_channels, tuple(z.shape)))
    if kind not in _KINDS:
        raise ValueError("kind must be VAE_DEC_SAMPLE, VAE_DEC_UNIT or VAE_DEC_U8 (got %r)" % (kind,))
    N, _, h, w = z.shape
    f = m.up_factor
    dt = m.dtype if out_dtype is None else out_dtype
    if kind == L.VAE_DEC_SAMPLE:
        shape, odt = (N, 3, h * f, w * f), dt
    elif kind == L.VAE_DEC_UNIT:
        shape, odt = (N, 3, h * f, w * f), torch.float32
    else:
        shape, odt = (N, h * f, w * f, 3), torch.uint8
    if out is None:
        out = torch.empty(shape, dtype=odt, device=dev)
    elif tuple(out.shape) != shape or out.dtype != odt or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor of shape %s on %s" % (odt, shape, dev))
    if N and (z.stride(3) != 1 or z.stride(2) != w or z.stride(1) < h * w):      # the head kernel reads dense [h][w] planes at any two strides
        z = z.contiguous()
    return dev, z, out, dt


def _run_decoder(m, plan, z, kind, scale, out_dtype, out=None):
    """one ctrl_vae_decoder_forward of the module `m` with the plan `plan`; `out`: a contiguous tensor of the result's shape and dtype to
    write into (a slice of a larger buffer) instead of a new one"""
    dev, z, out, dt = _decoder_io(m, z, kind, out_dtype, out)
    N, _, h, w = z.shape
    if N == 0:
        return out
    with torch.cuda.device(dev):
        L.check(L.lib().ctrl_vae_decoder_forward_strided(plan(), L.ptr(z), L.dtype_code(z.dtype), N, h, w, z.stride(0), z.stride(1),
                                                         float(scale), int(kind), L.ptr(out), L.dtype_code(dt), L.cur_stream()))
    L.raise_if_out_of_range(type(m).__name__)
    return out


class AutoencoderKLDecoder(ParamTreeModule):
    """The decoder of diffusers' AutoencoderKL (its config kwargs; the encoder is AutoencoderKLEncoder, both are AutoencoderKL).  An
    image's pixels are bit-identical alone or inside any batch."""

    _CREATE, _DESTROY = "ctrl_vae_decoder_create", "ctrl_vae_decoder_destroy"

    def __init__(self, in_channels=3, out_channels=3, down_block_types=None, up_block_types=None,
                 block_out_channels=(128, 256, 512, 512), layers_per_block=2, act_fn="silu", latent_channels=4, norm_num_groups=32,
                 sample_size=512, scaling_factor=0.18215, shift_factor=None, latents_mean=None, latents_std=None, force_upcast=True,
                 use_quant_conv=True, use_post_quant_conv=True, mid_block_add_attention=True, **unused):
        super().__init__()
        block_out_channels = tuple(int(c) for c in block_out_channels)
        if up_block_types is None:
            up_block_types = ("UpDecoderBlock2D",) * len(block_out_channels)
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__", "unused")})
        _check_vae_config("AutoencoderKLDecoder", "decoder", out_channels, up_block_types, block_out_channels, layers_per_block, act_fn,
                          latent_channels, norm_num_groups, use_post_quant_conv, mid_block_add_attention)
        self._cfg = _vae_config(block_out_channels, layers_per_block, latent_channels, norm_num_groups, out_channels)
        self.latent_channels = latent_channels
        self.up_factor = 2 ** (len(block_out_channels) - 1)
        self._register_spec(vae_decoder_spec(self._cfg), dtype=torch.float32)

    def config_dict(self):
        return dict(self.config)

    def load_state_dict(self, state_dict, strict=True, **k):
        """diffusers' keys of a whole VAE (encoder.* / quant_conv.* dropped), legacy attention names mapped"""
        return super().load_state_dict(_map_vae_keys(state_dict, ("encoder.", "quant_conv.")), strict=strict, **k)

    def run(self, z, kind=L.VAE_DEC_SAMPLE, scale=1.0, out_dtype=None, out=None):
        """one ctrl_vae_decoder_forward: z [N, lat, h, w] fp32 / fp16 / bf16 on the GPU, multiplied by `scale` on load -> kind
        VAE_DEC_SAMPLE: [N, 3, H, W] in out_dtype (default: the module's dtype) = decode(z * scale).sample; VAE_DEC_UNIT: fp32
        [N, 3, H, W] = (sample / 2 + 0.5).clamp(0, 1); VAE_DEC_U8: uint8 [N, H, W, 3] = round(that * 255).  For the last two out_dtype
        names the format `sample` is rounded to first.  `out`: a contiguous tensor of the result's shape to write into."""
        return _run_decoder(self, self._ensure_plan, z, kind, scale, out_dtype, out)

    def decode(self, z, return_dict=True, generator=None):
        sample = self.run(z, L.VAE_DEC_SAMPLE)
        return DecoderOutput(sample) if return_dict else (sample,)

    def forward(self, z, return_dict=True):
        return self.decode(z, return_dict=return_dict)


class AutoencoderKL(AutoencoderKLEncoder):
    """diffusers' AutoencoderKL over one set of parameters (the whole VAE's state-dict keys, unprefixed) and both libctrlhip plans:
    encode(x).latent_dist runs the encoder plan, decode(z).sample the decoder plan.  `config.force_upcast` reads False whatever the
    checkpoint says: the fp32 residual stream makes the SDXL pipeline's fp32 round trip (upcast_vae) unnecessary."""

    _WHO = "AutoencoderKL"

    def __init__(self, in_channels=3, out_channels=3, down_block_types=None, up_block_types=None,
                 block_out_channels=(128, 256, 512, 512), layers_per_block=2, act_fn="silu", latent_channels=4, norm_num_groups=32,
                 sample_size=512, scaling_factor=0.18215, shift_factor=None, latents_mean=None, latents_std=None, force_upcast=True,
                 use_quant_conv=True, use_post_quant_conv=True, mid_block_add_attention=True, **unused):
        boc = tuple(int(c) for c in block_out_channels)
        if up_block_types is None:
            up_block_types = ("UpDecoderBlock2D",) * len(boc)
        super().__init__(in_channels=in_channels, out_channels=out_channels, down_block_types=down_block_types,
                         up_block_types=up_block_types, block_out_channels=boc, layers_per_block=layers_per_block, act_fn=act_fn,
                         latent_channels=latent_channels, norm_num_groups=norm_num_groups, sample_size=sample_size,
                         scaling_factor=scaling_factor, shift_factor=shift_factor, latents_mean=latents_mean,
                         latents_std=latents_std, force_upcast=force_upcast, use_quant_conv=use_quant_conv,
                         use_post_quant_conv=use_post_quant_conv, mid_block_add_attention=mid_block_add_attention)
        _check_vae_config("AutoencoderKL", "decoder", out_channels, up_block_types, boc, layers_per_block, act_fn, latent_channels,
                          norm_num_groups, use_post_quant_conv, mid_block_add_attention)
        self._dec_plan = None
        self.config["force_upcast"] = False
        self._dec_cfg = _vae_config(boc, layers_per_block, latent_channels, norm_num_groups, out_channels)
        self.up_factor = 2 ** (len(boc) - 1)
        enc_spec = self._spec
        dec_spec = vae_decoder_spec(self._dec_cfg)
        self._register_spec(dec_spec, dtype=torch.float32)
        self._spec = list(enc_spec) + list(dec_spec)

    def load_state_dict(self, state_dict, strict=True, **k):
        """the whole VAE's keys; legacy attention names of both halves mapped"""
        return ParamTreeModule.load_state_dict(self, _map_vae_keys(state_dict, (), ("encoder", "decoder")), strict=strict, **k)

    def _drop_plan(self):
        if getattr(self, "_dec_plan", None) is not None:
            L.lib().ctrl_vae_decoder_destroy(self._dec_plan)
        self._dec_plan = None
        super()._drop_plan()

    def _ensure_dec_plan(self):
        return self._ensure_plan("_dec_plan", "ctrl_vae_decoder_create", ("_dec_cfg",))

    def run_decoder(self, z, kind=L.VAE_DEC_SAMPLE, scale=1.0, out_dtype=None, out=None):
        """AutoencoderKLDecoder.run on this module's decoder plan"""
        return _run_decoder(self, self._ensure_dec_plan, z, kind, scale, out_dtype, out)

    def decode(self, z, return_dict=True, generator=None):
        sample = self.run_decoder(z, L.VAE_DEC_SAMPLE)
        return DecoderOutput(sample) if return_dict else (sample,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        dist = self.encode(sample).latent_dist
        z = dist.sample(generator=generator) if sample_posterior else dist.mode()
        return self.decode(z, return_dict=return_dict)


def _decoder_run_of(vae):
    """the mirror's one-forward entry (run of the decoder, run_decoder of the whole VAE), or None for a torch VAE"""
    if isinstance(vae, AutoencoderKLDecoder):
        return vae.run
    if isinstance(vae, AutoencoderKL):
        return vae.run_decoder
    return None


def _numpy_to_pil(images):
    from PIL import Image
    if images.shape[-1] == 1:
        return [Image.fromarray(im.squeeze(), mode="L") for im in images]
    return [Image.fromarray(im) for im in images]


@torch.no_grad()
def decode_sdxl_latents(vae, latents, output_type="pil"):
    """The SDXL pipeline's final decode (sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1406-1427, without the watermark) with the VAE
    passed in: vae.decode(latents / scaling_factor) then VaeImageProcessor.postprocess -- "latent": the latents; "pt": fp-valued
    [N, 3, H, W] in [0, 1]; "np": the same as an NHWC float32 array; "pil": a list of PIL images.  On the mirror it is ONE forward with
    scale = 1 / scaling_factor and the matching epilogue (no upcast: the stream is fp32); on a torch VAE it takes the pipeline's route,
    the fp32 round trip under force_upcast included."""
    if output_type == "latent":
        return latents
    if output_type not in ("pt", "np", "pil"):
        raise ValueError("output_type must be latent, pt, np or pil (got %r)" % (output_type,))
    sf = _scaling_factor(vae)
    run = _decoder_run_of(vae)
    if run is not None:
        if output_type == "pil":
            return _numpy_to_pil(run(latents, L.VAE_DEC_U8, scale=1.0 / sf).cpu().numpy())
        image = run(latents, L.VAE_DEC_UNIT, scale=1.0 / sf)
        return image if output_type == "pt" else image.cpu().permute(0, 2, 3, 1).float().numpy()
    cfg = vae.config
    force = cfg["force_upcast"] if isinstance(cfg, dict) else cfg.force_upcast
    needs_upcasting = vae.dtype == torch.float16 and force
    if needs_upcasting:
        vae.to(dtype=torch.float32)
        latents = latents.to(torch.float32)
    image = vae.decode(latents / sf, return_dict=False)[0]
    if needs_upcasting:
        vae.to(dtype=torch.float16)
    image = (image / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return image
    image = image.cpu().permute(0, 2, 3, 1).float().numpy()
    if output_type == "np":
        return image
    return _numpy_to_pil((image * 255).round().astype("uint8"))


@torch.no_grad()
def decode_i2vgen_latents(vae, latents, decode_chunk_size=None):
    """The I2VGen-XL pipeline's decode_latents (i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:398-418) with the VAE passed
    in: [B, C, F, h, w] latents / scaling_factor, frames decoded decode_chunk_size at a time -> [B, 3, F, H, W] float32 (as the
    pipeline's, a permuted view of the [B, F, 3, H, W] frames).  On the mirror the (batch, frame) permute is the strides of the forward:
    clip b is one call over its F frames as the [F, C, h, w] view of latents[b] (image stride h * w, channel stride F * h * w) that
    writes frames[b], 1 / scaling_factor rides on the head kernel's load, and no copy of the latents is made.  The plan decodes image
    after image whatever the batch, so decode_chunk_size changes nothing there."""
    B, Cl, F, h, w = latents.shape
    sf = _scaling_factor(vae)
    run = _decoder_run_of(vae)
    if run is not None:
        f = vae.up_factor
        frames = torch.empty((B, F, 3, h * f, w * f), dtype=vae.dtype, device=latents.device)
        for b in range(B):
            run(latents[b].transpose(0, 1), L.VAE_DEC_SAMPLE, scale=1.0 / sf, out=frames[b])
        return frames.permute(0, 2, 1, 3, 4).float()
    latents = 1 / sf * latents
    latents = latents.permute(0, 2, 1, 3, 4).reshape(B * F, Cl, h, w)
    if decode_chunk_size is not None:
        frames = [vae.decode(latents[i:i + decode_chunk_size]).sample for i in range(0, latents.shape[0], decode_chunk_size)]
        image = torch.cat(frames, dim=0)
    else:
        image = vae.decode(latents).sample
    video = image[None, :].reshape((B, F, -1) + image.shape[2:]).permute(0, 2, 1, 3, 4)
    return video.float()
