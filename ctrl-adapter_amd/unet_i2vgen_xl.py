"""I2VGenXLUNet -- I2VGen-XL's frozen backbone UNet as the reference extends it with the two ControlNet-residual kwargs
(i2vgen_xl/models/unets/unet_i2vgen_xl.py: constructor :134-322, forward :519-761), a drop-in for `pipe.unet` of the I2VGen-XL pipeline
whose forward runs in libctrlhip (csrc/plan_unet_i2v.cpp, csrc/unet.hip).  Same constructor arguments, same forward signature, the
reference's state-dict keys.  The adapter's residuals go in as the adapter returns them, `(b f) c h w` or the 5-D `b c f h w`, in
fp32 / fp16 / bf16: the up path's skip join reads them in place.  `cache_condition = True` keeps what depends on
encoder_hidden_states, image_latents and image_embeddings only (every cross-attention's K / V, the encoded latent channels) across the
denoise steps of a request.  There is no CPU path."""
import ctypes as C

import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec, timesteps_to_device_f32

_WHO = "I2VGenXLUNet (libctrlhip): "
_DOWN = ("CrossAttnDownBlock3D", "DownBlock3D")
_UP = ("CrossAttnUpBlock3D", "UpBlock3D")
MAX_FRAMES = 32      # ctrl_op_temporal_attn's sequence limit
COND_OFF, COND_KEEP, COND_REUSE = 0, 1, 2


class UNet3DConditionOutput(tuple):
    """(sample,) with attribute access, as diffusers' UNet3DConditionOutput"""

    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


def unet_i2v_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, layers_per_block, norm_num_groups,
                    cross_attention_dim, attention_head_dim):
    """the ctrl_unet_i2v_config of the reference's constructor arguments; refuses what the plan does not run"""
    down, up, boc = tuple(down_block_types), tuple(up_block_types), tuple(int(c) for c in block_out_channels)
    n = len(down)
    if len(up) != n or len(boc) != n:
        raise ValueError(_WHO + "must provide the same number of `down_block_types`, `up_block_types` and `block_out_channels`")
    if not 1 <= n <= 4:
        raise ValueError(_WHO + "1 .. 4 levels are supported (got %d)" % n)
    bad = [t for t in down if t not in _DOWN] + [t for t in up if t not in _UP]
    if bad:
        raise ValueError(_WHO + "unsupported block type(s) %s in `down_block_types` / `up_block_types`: %s / %s are the ones that run here"
                         % (sorted(set(bad)), _DOWN, _UP))
    attn = [t == _DOWN[0] for t in down]
    if [t == _UP[0] for t in up] != attn[::-1]:
        raise ValueError(_WHO + "`up_block_types` must mirror `down_block_types` (attention at the same levels)")
    if int(in_channels) != 4:
        raise ValueError(_WHO + "`in_channels` = %r: the latent stems and the temporal encoder are built for 4 channels" % (in_channels,))
    if norm_num_groups != 32:
        raise ValueError(_WHO + "`norm_num_groups` = %r: the GroupNorm kernels run 32 groups" % (norm_num_groups,))
    # the reference reads the head DIMENSION from attention_head_dim (and ignores num_attention_heads): every level has C / 64 heads
    hd = attention_head_dim if isinstance(attention_head_dim, int) else tuple(attention_head_dim)
    if hd != 64 and hd != (64,) * n:
        raise ValueError(_WHO + "`attention_head_dim` = %r: the attention kernels run heads of 64" % (attention_head_dim,))
    if not isinstance(layers_per_block, int) or not isinstance(cross_attention_dim, int):
        raise ValueError(_WHO + "`layers_per_block` and `cross_attention_dim` must be plain ints")
    cfg = L.UNetI2VConfig()
    cfg.in_channels, cfg.out_channels, cfg.num_levels = int(in_channels), int(out_channels), n
    for i in range(n):
        cfg.block_out_channels[i] = boc[i]
        cfg.level_has_attn[i] = int(attn[i])
    cfg.layers_per_block, cfg.cross_attention_dim = layers_per_block, cross_attention_dim
    return cfg


def unet_i2v_spec(cfg):
    """(name, shape) of every parameter of a ctrl_unet_i2v_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_unet_i2v_param_count, lib.ctrl_unet_i2v_param_spec, cfg)


class I2VGenXLUNet(ParamTreeModule):
    _CREATE, _DESTROY = "ctrl_unet_i2v_create", "ctrl_unet_i2v_destroy"

    def __init__(self, sample_size=None, in_channels=4, out_channels=4,
                 down_block_types=("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
                 up_block_types=("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"),
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, norm_num_groups=32, cross_attention_dim=1024,
                 attention_head_dim=64, num_attention_heads=None):
        super().__init__()
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__")})
        self._cfg = unet_i2v_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, layers_per_block,
                                    norm_num_groups, cross_attention_dim, attention_head_dim)
        self._register_spec(unet_i2v_spec(self._cfg), dtype=torch.float32)
        # skip i of the down path: (channels, down-sampling factor), transformer_in's output first
        n, boc, lpb = self._cfg.num_levels, list(self._cfg.block_out_channels), self._cfg.layers_per_block
        self._skips = [(boc[0], 1)]
        for i in range(n):
            self._skips += [(boc[i], 2 ** i)] * lpb + ([(boc[i], 2 ** (i + 1))] if i + 1 < n else [])
        self._mid = (boc[n - 1], 2 ** (n - 1))
        self.cache_condition = False
        self._force_cond_mode = None          # tests: COND_* for the next forwards, whatever the inputs are
        self._cond_key, self._cond_mode = None, COND_OFF

    def config_dict(self):
        return {k: (list(v) if isinstance(v, tuple) else v) for k, v in self.config.items()}

    def load_state_dict(self, state_dict, *a, **k):
        # diffusers' Transformer2DModel held its projections as 1x1 convolutions before they became linear: [C, C, 1, 1] is accepted
        sd = dict(state_dict)
        for name, v in list(sd.items()):
            if name.endswith((".proj_in.weight", ".proj_out.weight")) and torch.is_tensor(v) and v.dim() == 4 and v.shape[2:] == (1, 1):
                sd[name] = v[:, :, 0, 0]
        return super().load_state_dict(sd, *a, **k)

    def _plan_created(self, slot):
        self._note_selection(L.lib().ctrl_unet_i2v_selection)

    def _drop_plan(self):
        super()._drop_plan()
        self._cond_key, self._cond_mode = None, COND_OFF          # the cache lives in the plan

    def workspace_bytes(self):
        """bytes of the plan's forward workspace (the largest forward so far); 0 before the first forward"""
        return int(L.lib().ctrl_unet_i2v_workspace_bytes(self._plan)) if self._plan is not None else 0

    def _residual(self, r, what, B, F, h, w, chans, factor, dev):
        """a residual as the skip join reads it: (tensor, is_5d) after the shape / device checks"""
        if not torch.is_tensor(r) or not r.is_cuda or r.device != dev:
            raise ValueError(_WHO + "%s must be a tensor on %s" % (what, dev))
        want4, want5 = (B * F, chans, h // factor, w // factor), (B, chans, F, h // factor, w // factor)
        if tuple(r.shape) not in (want4, want5):
            raise ValueError(_WHO + "%s has shape %s, expected %s or %s" % (what, tuple(r.shape), want4, want5))
        L.dtype_code(r.dtype)
        return r.contiguous(), r.dim() == 5

    def _cond_cache_mode(self, shape_key, tensors):
        """keep / reuse for this forward from the identity + version counter of the three condition tensors (the same, unmodified
        tensor objects come back on every denoise step of a request), told to the plan"""
        mode = COND_OFF
        if self._force_cond_mode is not None:
            mode = self._force_cond_mode
        elif self.cache_condition:
            key = shape_key + tuple((id(t), t._version, t.data_ptr(), tuple(t.shape), t.dtype) for t in tensors)
            mode = COND_REUSE if key == self._cond_key else COND_KEEP
            self._cond_key, self._cond_refs = key, tensors        # (the references keep the ids from being recycled)
        if mode != self._cond_mode or mode:
            L.check(L.lib().ctrl_unet_i2v_set_cond_cache(self._ensure_plan(), mode))
            self._cond_mode = mode
        return mode

    def _check_args(self, sample, image_latents, image_embeddings, encoder_hidden_states, timestep_cond, cross_attention_kwargs):
        """the argument checks of forward that need no GPU"""
        if timestep_cond is not None:
            raise ValueError(_WHO + "`timestep_cond` is not supported by the plan (pass None)")
        if cross_attention_kwargs:
            raise ValueError(_WHO + "`cross_attention_kwargs` must be empty (got keys %s)" % sorted(cross_attention_kwargs))
        if image_embeddings is None:
            raise ValueError(_WHO + "`image_embeddings` is required (the context's image tokens)")
        if encoder_hidden_states is None:
            raise ValueError(_WHO + "`encoder_hidden_states` is required (the context's text tokens)")
        ic, cross = self._cfg.in_channels, self._cfg.cross_attention_dim
        if sample.dim() != 5 or sample.shape[1] != ic:
            raise ValueError(_WHO + "the sample must be [batch, %d, frames, h, w] (got %s)" % (ic, tuple(sample.shape)))
        B, _, F, h, w = sample.shape
        if F > MAX_FRAMES:
            raise ValueError(_WHO + "%d frames in `sample`: at most %d frames per clip (the temporal attention's limit)" % (F, MAX_FRAMES))
        m = 2 ** (self._cfg.num_levels - 1)
        if h % m or w % m or h < m or w < m:
            raise ValueError(_WHO + "the latent height and width of `sample` must be multiples of %d (got %d x %d)" % (m, h, w))
        if tuple(image_latents.shape) != (B, 4, F, h, w):
            raise ValueError(_WHO + "`image_latents` must be %s (got %s)" % ((B, 4, F, h, w), tuple(image_latents.shape)))
        if tuple(image_embeddings.shape) != (B, cross):
            raise ValueError(_WHO + "`image_embeddings` must be %s (got %s)" % ((B, cross), tuple(image_embeddings.shape)))
        ehs = encoder_hidden_states
        if ehs.dim() != 3 or ehs.shape[0] != B or ehs.shape[2] != cross or ehs.shape[1] < 1:
            raise ValueError(_WHO + "`encoder_hidden_states` must be [%d, tokens, %d] (got %s)" % (B, cross, tuple(ehs.shape)))
        return B, F, h, w

    @torch.no_grad()
    def forward(self, sample, timestep, fps, image_latents, image_embeddings=None, encoder_hidden_states=None, timestep_cond=None,
                cross_attention_kwargs=None, down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict=True):
        B, F, h, w = self._check_args(sample, image_latents, image_embeddings, encoder_hidden_states, timestep_cond, cross_attention_kwargs)
        dev = _check_gpu_input(self, sample, "the sample")
        for what, v in (("image_latents", image_latents), ("image_embeddings", image_embeddings),
                        ("encoder_hidden_states", encoder_hidden_states)):
            _check_gpu_input(self, v, "`%s`" % what)
            L.dtype_code(v.dtype)
        sample = sample.contiguous()
        lat, emb, ehs = image_latents.contiguous(), image_embeddings.contiguous(), encoder_hidden_states.contiguous()
        t = timesteps_to_device_f32(timestep, B, dev)
        fps_t = timesteps_to_device_f32(fps, B, dev)
        down, down_5d, down_dt = [], False, L.F32
        if down_block_additional_residuals is not None and len(down_block_additional_residuals):
            # zip(): skip i takes residual i; the list may be shorter than the skips (the rest stay as they are), never longer
            res = list(down_block_additional_residuals)
            if len(res) > len(self._skips):
                raise ValueError(_WHO + "%d down_block_additional_residuals for %d skips" % (len(res), len(self._skips)))
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
        out = torch.empty((B, self._cfg.out_channels, F, h, w), dtype=sample.dtype, device=dev)
        ptrs = (C.c_void_p * max(len(down), 1))()
        for i, r in enumerate(down):
            ptrs[i] = r.data_ptr()
        with torch.cuda.device(dev):
            self._cond_cache_mode((B, F, h, w), (encoder_hidden_states, image_latents, image_embeddings))
            L.check(L.lib().ctrl_unet_i2v_forward(self._ensure_plan(), L.ptr(sample), L.dtype_code(sample.dtype), B, F, h, w, L.ptr(t),
                                                  t.numel(), L.ptr(fps_t), fps_t.numel(), L.ptr(lat), L.dtype_code(lat.dtype), L.ptr(emb),
                                                  L.dtype_code(emb.dtype), L.ptr(ehs), L.dtype_code(ehs.dtype), ehs.shape[1], ptrs, len(down),
                                                  down_dt, int(down_5d), L.ptr(mid), mid_dt, int(mid_5d), L.ptr(out), L.cur_stream()))
        L.raise_if_out_of_range(type(self).__name__)
        return UNet3DConditionOutput(out) if return_dict else (out,)
