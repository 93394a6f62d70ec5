"""UNetSpatioTemporalConditionModel -- SVD's frozen backbone UNet as the reference extends it with the two ControlNet-residual
kwargs (svd/models/unets/unet_spatio_temporal_condition.py: constructor :70-246, forward :357-526), a drop-in for `pipe.unet` whose
forward runs in libctrlhip (csrc/plan_unet_st.cpp, csrc/unet.hip).  Same constructor arguments, same forward signature, diffusers'
state-dict keys.  The adapter's residuals go in as the adapter returns them, `(b f) c h w` or the 5-D `b c f h w` of `scatter_to=`,
in fp32 / fp16 / bf16: the up path's skip join reads them in place.  There is no CPU path."""
import ctypes as C

import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec, timesteps_to_device_f32

_WHO = "UNetSpatioTemporalConditionModel (libctrlhip): "
_DOWN = ("CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal")
_UP = ("CrossAttnUpBlockSpatioTemporal", "UpBlockSpatioTemporal")
MAX_FRAMES = 32      # ctrl_op_temporal_attn's sequence limit


class UNetSpatioTemporalConditionOutput(tuple):
    """(sample,) with attribute access, as diffusers' UNetSpatioTemporalConditionOutput"""

    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


def _per_level(v, n, what):
    if isinstance(v, int):
        return (v,) * n
    v = tuple(int(x) for x in v)
    if len(v) != n:
        raise ValueError(_WHO + "must provide the same number of `%s` as `down_block_types` (%d), got %d" % (what, n, len(v)))
    return v


def unet_st_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, addition_time_embed_dim,
                   projection_class_embeddings_input_dim, layers_per_block, cross_attention_dim, transformer_layers_per_block,
                   num_attention_heads, num_frames):
    """the ctrl_unet_st_config of the reference's constructor arguments; refuses what the plan does not run"""
    down, up, boc = tuple(down_block_types), tuple(up_block_types), tuple(int(c) for c in block_out_channels)
    n = len(down)
    if len(up) != n or len(boc) != n:
        raise ValueError(_WHO + "must provide the same number of `down_block_types`, `up_block_types` and `block_out_channels`")
    if not 1 <= n <= 4:
        raise ValueError(_WHO + "1 .. 4 levels are supported (got %d)" % n)
    bad = [t for t in down if t not in _DOWN] + [t for t in up if t not in _UP]
    if bad:
        raise ValueError(_WHO + "unsupported block type(s) %s: SVD's %s / %s are the ones that run here" % (sorted(set(bad)), _DOWN, _UP))
    attn = [t == _DOWN[0] for t in down]
    if [t == _UP[0] for t in up] != attn[::-1]:
        raise ValueError(_WHO + "the up blocks must mirror the down blocks (attention at the same levels)")
    heads = _per_level(num_attention_heads, n, "num_attention_heads")
    lpb = _per_level(layers_per_block, n, "layers_per_block")
    tlpb = _per_level(transformer_layers_per_block, n, "transformer_layers_per_block")
    cross = _per_level(cross_attention_dim, n, "cross_attention_dim")
    if len(set(lpb)) != 1 or len(set(tlpb)) != 1 or len(set(cross)) != 1:
        raise ValueError(_WHO + "layers_per_block, transformer_layers_per_block and cross_attention_dim must be the same at every level")
    for i in range(n):
        if (attn[i] or i == n - 1) and (heads[i] < 1 or boc[i] // heads[i] != 64 or boc[i] % heads[i]):
            raise ValueError(_WHO + "attention_head_dim = out_channels // num_attention_heads must be 64 (level %d: %d // %d)"
                             % (i, boc[i], heads[i]))
    if int(num_frames) > MAX_FRAMES:
        raise ValueError(_WHO + "num_frames = %d: at most %d frames per clip (the temporal attention's limit)" % (num_frames, MAX_FRAMES))
    cfg = L.UNetSTConfig()
    cfg.in_channels, cfg.out_channels, cfg.num_levels = int(in_channels), int(out_channels), n
    for i in range(n):
        cfg.block_out_channels[i] = boc[i]
        cfg.num_attention_heads[i] = heads[i]
        cfg.level_has_attn[i] = int(attn[i])
    cfg.layers_per_block, cfg.transformer_layers_per_block, cfg.cross_attention_dim = lpb[0], tlpb[0], cross[0]
    cfg.addition_time_embed_dim = int(addition_time_embed_dim)
    cfg.projection_class_embeddings_input_dim = int(projection_class_embeddings_input_dim)
    return cfg


def unet_st_spec(cfg):
    """(name, shape) of every parameter of a ctrl_unet_st_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_unet_st_param_count, lib.ctrl_unet_st_param_spec, cfg)


class UNetSpatioTemporalConditionModel(ParamTreeModule):
    _CREATE, _DESTROY = "ctrl_unet_st_create", "ctrl_unet_st_destroy"

    def __init__(self, sample_size=None, in_channels=8, out_channels=4,
                 down_block_types=("CrossAttnDownBlockSpatioTemporal", "CrossAttnDownBlockSpatioTemporal",
                                   "CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"),
                 up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal",
                                 "CrossAttnUpBlockSpatioTemporal"),
                 block_out_channels=(320, 640, 1280, 1280), addition_time_embed_dim=256, projection_class_embeddings_input_dim=768,
                 layers_per_block=2, cross_attention_dim=1024, transformer_layers_per_block=1, num_attention_heads=(5, 10, 10, 20),
                 num_frames=25):
        super().__init__()
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__")})
        self._cfg = unet_st_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, addition_time_embed_dim,
                                   projection_class_embeddings_input_dim, layers_per_block, cross_attention_dim,
                                   transformer_layers_per_block, num_attention_heads, num_frames)
        self._register_spec(unet_st_spec(self._cfg), dtype=torch.float32)
        # skip i of the down path: (channels, down-sampling factor), conv_in's output first
        n, boc, lpb = self._cfg.num_levels, list(self._cfg.block_out_channels), self._cfg.layers_per_block
        self._skips = [(boc[0], 1)]
        for i in range(n):
            self._skips += [(boc[i], 2 ** i)] * lpb + ([(boc[i], 2 ** (i + 1))] if i + 1 < n else [])
        self._mid = (boc[n - 1], 2 ** (n - 1))

    def config_dict(self):
        return {k: (list(v) if isinstance(v, tuple) else v) for k, v in self.config.items()}

    def _plan_created(self, slot):
        self._note_selection(L.lib().ctrl_unet_st_selection)

    def _residual(self, r, what, B, F, h, w, chans, factor, dev):
        """a residual as the skip join reads it: (tensor, is_5d) after the shape / device checks"""
        if not torch.is_tensor(r) or not r.is_cuda or r.device != dev:
            raise ValueError(_WHO + "%s must be a tensor on %s" % (what, dev))
        want4, want5 = (B * F, chans, h // factor, w // factor), (B, chans, F, h // factor, w // factor)
        if tuple(r.shape) not in (want4, want5):
            raise ValueError(_WHO + "%s has shape %s, expected %s or %s" % (what, tuple(r.shape), want4, want5))
        L.dtype_code(r.dtype)
        return r.contiguous(), r.dim() == 5

    @torch.no_grad()
    def forward(self, sample, timestep, encoder_hidden_states, added_time_ids, down_block_additional_residuals=None,
                mid_block_additional_residual=None, return_dict=True):
        dev = _check_gpu_input(self, sample, "the sample")
        if sample.dim() != 5 or sample.shape[2] != self._cfg.in_channels:
            raise ValueError(_WHO + "the sample must be [batch, frames, %d, h, w] (got %s)" % (self._cfg.in_channels, tuple(sample.shape)))
        B, F, _, h, w = sample.shape
        if F > MAX_FRAMES:
            raise ValueError(_WHO + "%d frames: at most %d frames per clip (the temporal attention's limit)" % (F, MAX_FRAMES))
        if h % 8 or w % 8:
            raise ValueError(_WHO + "the latent height and width must be multiples of 8 (got %d x %d)" % (h, w))
        ehs = encoder_hidden_states
        cross = self._cfg.cross_attention_dim
        if ehs.dim() != 3 or ehs.shape[0] != B or ehs.shape[2] != cross:
            raise ValueError(_WHO + "encoder_hidden_states must be [%d, 1, %d] (got %s)" % (B, cross, tuple(ehs.shape)))
        if ehs.shape[1] != 1:
            raise ValueError(_WHO + "encoder_hidden_states with %d keys: the plan runs SVD's single image embedding ([batch, 1, %d])"
                             % (ehs.shape[1], cross))
        n_ids = self._cfg.projection_class_embeddings_input_dim // self._cfg.addition_time_embed_dim
        if added_time_ids.dim() != 2 or tuple(added_time_ids.shape) != (B, n_ids):
            raise ValueError(_WHO + "added_time_ids must be [%d, %d] (got %s)" % (B, n_ids, tuple(added_time_ids.shape)))
        sample = sample.contiguous()
        ehs = ehs.to(dev).contiguous()
        t = timesteps_to_device_f32(timestep, B, dev)
        ids = added_time_ids.detach().to(device=dev, dtype=torch.float32).contiguous()
        down, down_5d, down_dt = [], False, L.F32
        if down_block_additional_residuals is not None and len(down_block_additional_residuals):
            # zip(): skip i takes residual i; the list may be shorter than the skips (the rest stay as they are), never longer
            res = list(down_block_additional_residuals)[:len(self._skips)]
            for i, r in enumerate(res):
                r, is5 = self._residual(r, "down_block_additional_residuals[%d]" % i, B, F, h, w, self._skips[i][0], self._skips[i][1], dev)
                down.append(r)
                if i == 0:
                    down_5d, down_dt = is5, L.dtype_code(r.dtype)
                elif is5 != down_5d or L.dtype_code(r.dtype) != down_dt:
                    raise ValueError(_WHO + "down_block_additional_residuals must share one layout (4-D or 5-D) and one dtype")
        mid, mid_5d, mid_dt = None, False, L.F32
        if mid_block_additional_residual is not None:
            mid, mid_5d = self._residual(mid_block_additional_residual, "mid_block_additional_residual", B, F, h, w, self._mid[0],
                                         self._mid[1], dev)
            mid_dt = L.dtype_code(mid.dtype)
        out = torch.empty((B, F, self._cfg.out_channels, h, w), dtype=sample.dtype, device=dev)
        ptrs = (C.c_void_p * max(len(down), 1))()
        for i, r in enumerate(down):
            ptrs[i] = r.data_ptr()
        with torch.cuda.device(dev):
            L.check(L.lib().ctrl_unet_st_forward(self._ensure_plan(), L.ptr(sample), L.dtype_code(sample.dtype), B, F, h, w, L.ptr(t),
                                                 t.numel(), L.ptr(ehs), L.dtype_code(ehs.dtype), L.ptr(ids), n_ids, ptrs, len(down),
                                                 down_dt, int(down_5d), L.ptr(mid), mid_dt, int(mid_5d), L.ptr(out), L.cur_stream()))
        L.raise_if_out_of_range(type(self).__name__)
        return UNetSpatioTemporalConditionOutput(out) if return_dict else (out,)
