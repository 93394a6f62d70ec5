"""AutoencoderKLTemporalDecoder -- diffusers' AutoencoderKLTemporalDecoder (v0.27: the KL-VAE encoder + quant_conv of vae_encoder.py and
a TemporalDecoder, no post_quant_conv) over one set of parameters, a drop-in for SVD's `pipe.vae`; its decode runs in libctrlhip
(csrc/plan_vae_tdecoder.cpp, csrc/vae.hip), and the SVD pipeline's decode step:

  decode_svd_latents  svd/pipelines/svd_controlnet_adapter_pipeline.py:265-292 (decode_latents: [B, F, C, h, w] latents /
                      scaling_factor, the flattened frames decoded decode_chunk_size at a time, every chunk as ONE clip
                      -> [B, 3, F, H, W] float32)

State-dict keys are diffusers' (`encoder.*`, `quant_conv.*`, `decoder.mid_block.resnets.0.spatial_res_block.conv1.weight`, ...,
`decoder.time_conv_out.bias`).  A plain AutoencoderKL checkpoint is refused here, as a temporal one is by AutoencoderKL."""
import inspect

import torch

from . import _lib as L
from ._plan import ParamTreeModule, c_spec
from .vae_decoder import DecoderOutput, _decoder_io
from .vae_encoder import AutoencoderKLEncoder, _check_vae_config, _map_vae_keys, _scaling_factor, _vae_config


def vae_tdecoder_spec(cfg):
    """(name, shape) of every decoder parameter of a ctrl_vae_decoder_config read as a temporal decoder, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_vae_tdecoder_param_count, lib.ctrl_vae_tdecoder_param_spec, cfg)


class AutoencoderKLTemporalDecoder(AutoencoderKLEncoder):
    """diffusers' AutoencoderKLTemporalDecoder (its config kwargs) over both libctrlhip plans: encode(x).latent_dist runs the encoder
    plan, decode(z, num_frames).sample the temporal decoder plan, created on first use.  A clip's pixels are bit-identical alone or
    beside other clips in one call.  `config.force_upcast` reads False whatever the checkpoint says: the residual stream is fp32."""

    _WHO = "AutoencoderKLTemporalDecoder"

    def __init__(self, in_channels=3, out_channels=3, down_block_types=None, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                 latent_channels=4, sample_size=768, scaling_factor=0.18215, force_upcast=True, **unused):
        boc = tuple(int(c) for c in block_out_channels)
        super().__init__(in_channels=in_channels, out_channels=out_channels, down_block_types=down_block_types, block_out_channels=boc,
                         layers_per_block=layers_per_block, latent_channels=latent_channels, sample_size=sample_size,
                         scaling_factor=scaling_factor, force_upcast=force_upcast)
        _check_vae_config(self._WHO, "decoder", out_channels, ("UpDecoderBlock2D",) * len(boc), boc, layers_per_block, "silu",
                          latent_channels, 32, True, True)
        self._dec_plan = None
        self.config["force_upcast"] = False
        self._dec_cfg = _vae_config(boc, layers_per_block, latent_channels, 32, out_channels)
        self.up_factor = 2 ** (len(boc) - 1)
        enc_spec = self._spec
        dec_spec = vae_tdecoder_spec(self._dec_cfg)
        self._register_spec(dec_spec, dtype=torch.float32)
        self._spec = list(enc_spec) + list(dec_spec)

    def load_state_dict(self, state_dict, strict=True, **k):
        """the whole VAE's keys (legacy attention names of the encoder mapped); a plain AutoencoderKL checkpoint is refused"""
        if not any(key.startswith("decoder.") and ".spatial_res_block." in key for key in state_dict):
            raise ValueError("this is not a temporal-decoder checkpoint (no decoder ... spatial_res_block keys): a plain KL-VAE loads into "
                             "AutoencoderKL, AutoencoderKLTemporalDecoder takes SVD's VAE")
        return ParamTreeModule.load_state_dict(self, _map_vae_keys(state_dict, (), ("encoder",)), strict=strict, **k)

    def _drop_plan(self):
        if getattr(self, "_dec_plan", None) is not None:
            L.lib().ctrl_vae_tdecoder_destroy(self._dec_plan)
        self._dec_plan = None
        super()._drop_plan()

    def _ensure_dec_plan(self):
        return self._ensure_plan("_dec_plan", "ctrl_vae_tdecoder_create", ("_dec_cfg",))

    def run_decoder(self, z, num_frames, kind=L.VAE_DEC_SAMPLE, scale=1.0, out_dtype=None, out=None, frames_per_launch=None):
        """one ctrl_vae_tdecoder_forward: z [B * num_frames, lat, h, w] fp32 / fp16 / bf16 on the GPU (clip after clip), multiplied by
        `scale` on load -> the frames in the same order, with AutoencoderKLDecoder.run's kinds (VAE_DEC_SAMPLE: [N, 3, H, W] in out_dtype;
        VAE_DEC_UNIT: fp32 [N, 3, H, W] in [0, 1]; VAE_DEC_U8: uint8 [N, H, W, 3]).  `out`: a contiguous tensor of the result's shape to
        write into; frames_per_launch: cap on the group of frames one launch covers (None: the largest the index widths allow)."""
        num_frames = int(num_frames)
        if num_frames < 1 or z.shape[0] % num_frames != 0:
            raise ValueError("the %d latent frames are not whole clips of num_frames = %d" % (z.shape[0], num_frames))
        fpl = 0 if frames_per_launch is None else int(frames_per_launch)
        if frames_per_launch is not None and fpl < 1:
            raise ValueError("frames_per_launch must be None or positive (got %r)" % (frames_per_launch,))
        dev, z, out, dt = _decoder_io(self, z, kind, out_dtype, out)
        N, _, h, w = z.shape
        if N == 0:
            return out
        with torch.cuda.device(dev):
            L.check(L.lib().ctrl_vae_tdecoder_forward(self._ensure_dec_plan(), L.ptr(z), L.dtype_code(z.dtype), N // num_frames, num_frames,
                                                      h, w, z.stride(0), z.stride(1), float(scale), int(kind), L.ptr(out),
                                                      L.dtype_code(dt), fpl, L.cur_stream()))
        L.raise_if_out_of_range(type(self).__name__)
        return out

    def decode(self, z, num_frames, return_dict=True):
        sample = self.run_decoder(z, num_frames, L.VAE_DEC_SAMPLE)
        return DecoderOutput(sample) if return_dict else (sample,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None, num_frames=1):
        dist = self.encode(sample).latent_dist
        z = dist.sample(generator=generator) if sample_posterior else dist.mode()
        return self.decode(z, num_frames=num_frames, return_dict=return_dict)


@torch.no_grad()
def decode_svd_latents(vae, latents, num_frames, decode_chunk_size=14):
    """The SVD pipeline's decode_latents (svd/pipelines/svd_controlnet_adapter_pipeline.py:265-292) with the VAE passed in: [B, F, C, h, w]
    latents / scaling_factor, the B * F flattened frames walked in chunks of decode_chunk_size, every chunk decoded as one clip of its
    own length (a chunk may straddle two clips, as in the pipeline) -> [B, 3, F, H, W] float32.  On the mirror a chunk is one forward
    with scale = 1 / scaling_factor that writes its slice of one [B * F, 3, H, W] buffer, and no copy of the latents is made; on a torch
    VAE it takes the pipeline's route (num_frames is passed where the VAE's forward has that parameter)."""
    sf = _scaling_factor(vae)
    flat = latents.flatten(0, 1)
    if isinstance(vae, AutoencoderKLTemporalDecoder):
        N, _, h, w = flat.shape
        f = vae.up_factor
        frames = torch.empty((N, 3, h * f, w * f), dtype=vae.dtype, device=flat.device)
        for i in range(0, N, decode_chunk_size):
            n = min(decode_chunk_size, N - i)
            vae.run_decoder(flat[i:i + n], n, L.VAE_DEC_SAMPLE, scale=1.0 / sf, out=frames[i:i + n])
    else:
        flat = 1 / sf * flat
        fwd = vae._orig_mod.forward if hasattr(vae, "_orig_mod") else vae.forward
        accepts_num_frames = "num_frames" in set(inspect.signature(fwd).parameters.keys())
        chunks = []
        for i in range(0, flat.shape[0], decode_chunk_size):
            kw = {"num_frames": flat[i:i + decode_chunk_size].shape[0]} if accepts_num_frames else {}
            chunks.append(vae.decode(flat[i:i + decode_chunk_size], **kw).sample)
        frames = torch.cat(chunks, dim=0)
    return frames.reshape(-1, num_frames, *frames.shape[1:]).permute(0, 2, 1, 3, 4).float()
