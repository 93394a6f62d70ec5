"""UNet2DConditionModel -- SDXL's frozen backbone UNet (diffusers' UNet2DConditionModel in the configuration family of SDXL-base:
addition_embed_type "text_time", linear transformer projections, a transformer depth per level), a drop-in for `pipe.unet` whose forward
runs in libctrlhip (csrc/plan_unet2d.cpp, csrc/unet.hip).  It is called at sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:1356-1366
and consumes the adapter's residuals as the adapter returns them (`b c h w`, fp32 / fp16 / bf16): the up path's skip join reads them in
place.  diffusers' constructor argument names, forward signature and state-dict keys.  There is no CPU path."""
import ctypes as C

import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec, timesteps_to_device_f32

_WHO = "UNet2DConditionModel (libctrlhip): "
_DOWN = ("CrossAttnDownBlock2D", "DownBlock2D")
_UP = ("CrossAttnUpBlock2D", "UpBlock2D")

# every key of SDXL-base's unet/config.json the plan has ONE value for: anything else is refused
_FIXED = dict(center_input_sample=False, flip_sin_to_cos=True, freq_shift=0, mid_block_type="UNetMidBlock2DCrossAttn",
              only_cross_attention=False, downsample_padding=1, mid_block_scale_factor=1, dropout=0.0, act_fn="silu", norm_num_groups=32,
              encoder_hid_dim=None, encoder_hid_dim_type=None, dual_cross_attention=False, use_linear_projection=True,
              class_embed_type=None, addition_embed_type="text_time", num_class_embeds=None, upcast_attention=(None, False),
              resnet_time_scale_shift="default", resnet_skip_time_act=False, resnet_out_scale_factor=1.0, time_embedding_type="positional",
              time_embedding_dim=None, time_embedding_act_fn=None, timestep_post_act=None, time_cond_proj_dim=None, conv_in_kernel=3,
              conv_out_kernel=3, class_embeddings_concat=False, mid_block_only_cross_attention=None, cross_attention_norm=None,
              addition_embed_type_num_heads=64, attention_type="default", reverse_transformer_layers_per_block=None)


class UNet2DConditionOutput(tuple):
    """(sample,) with attribute access, as diffusers' UNet2DConditionOutput"""

    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


def _per_level(v, n, what):
    if isinstance(v, int):
        return (v,) * n
    v = tuple(v)
    if any(not isinstance(x, int) for x in v):
        raise ValueError(_WHO + "`%s` must be an int or one int per level (got %r)" % (what, v))
    if len(v) != n:
        raise ValueError(_WHO + "must provide the same number of `%s` as `down_block_types` (%d), got %d" % (what, n, len(v)))
    return v


def unet2d_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, layers_per_block,
                  transformer_layers_per_block, heads, cross_attention_dim, addition_time_embed_dim,
                  projection_class_embeddings_input_dim, norm_eps):
    """the ctrl_unet2d_config of diffusers' constructor arguments; refuses what the plan does not run"""
    down, up, boc = tuple(down_block_types), tuple(up_block_types), tuple(int(c) for c in block_out_channels)
    n = len(down)
    if len(up) != n or len(boc) != n:
        raise ValueError(_WHO + "must provide the same number of `down_block_types`, `up_block_types` and `block_out_channels`")
    if not 1 <= n <= 4:
        raise ValueError(_WHO + "1 .. 4 levels are supported (got %d)" % n)
    bad = [t for t in down if t not in _DOWN] + [t for t in up if t not in _UP]
    if bad:
        raise ValueError(_WHO + "unsupported block type(s) %s: %s / %s are the ones that run here" % (sorted(set(bad)), _DOWN, _UP))
    attn = [t == _DOWN[0] for t in down]
    if [t == _UP[0] for t in up] != attn[::-1]:
        raise ValueError(_WHO + "the up blocks must mirror the down blocks (attention at the same levels)")
    heads = _per_level(heads, n, "num_attention_heads / attention_head_dim")
    tlpb = _per_level(transformer_layers_per_block, n, "transformer_layers_per_block")
    if not isinstance(layers_per_block, int) or not isinstance(cross_attention_dim, int):
        raise ValueError(_WHO + "layers_per_block and cross_attention_dim must be the same at every level (plain ints)")
    for i in range(n):
        if (attn[i] or i == n - 1) and (heads[i] < 1 or boc[i] % heads[i] or boc[i] // heads[i] != 64):
            raise ValueError(_WHO + "out_channels // heads must be 64 at every attention level and in the mid block (level %d: %d // %d)"
                             % (i, boc[i], heads[i]))
    cfg = L.UNet2DConfig()
    cfg.in_channels, cfg.out_channels, cfg.num_levels = int(in_channels), int(out_channels), n
    for i in range(n):
        cfg.block_out_channels[i] = boc[i]
        cfg.num_attention_heads[i] = heads[i]
        cfg.transformer_layers_per_block[i] = tlpb[i]
        cfg.level_has_attn[i] = int(attn[i])
    cfg.layers_per_block, cfg.cross_attention_dim = layers_per_block, cross_attention_dim
    cfg.addition_time_embed_dim = int(addition_time_embed_dim)
    cfg.projection_class_embeddings_input_dim = int(projection_class_embeddings_input_dim)
    cfg.norm_eps = float(norm_eps)
    return cfg


def unet2d_spec(cfg):
    """(name, shape) of every parameter of a ctrl_unet2d_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_unet2d_param_count, lib.ctrl_unet2d_param_spec, cfg)


class UNet2DConditionModel(ParamTreeModule):
    _CREATE, _DESTROY = "ctrl_unet2d_create", "ctrl_unet2d_destroy"

    def __init__(self, sample_size=None, in_channels=4, out_channels=4, center_input_sample=False, flip_sin_to_cos=True, freq_shift=0,
                 down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                 mid_block_type="UNetMidBlock2DCrossAttn",
                 up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), only_cross_attention=False,
                 block_out_channels=(320, 640, 1280), layers_per_block=2, downsample_padding=1, mid_block_scale_factor=1, dropout=0.0,
                 act_fn="silu", norm_num_groups=32, norm_eps=1e-5, cross_attention_dim=2048, transformer_layers_per_block=(1, 2, 10),
                 reverse_transformer_layers_per_block=None, encoder_hid_dim=None, encoder_hid_dim_type=None,
                 attention_head_dim=(5, 10, 20), num_attention_heads=None, dual_cross_attention=False, use_linear_projection=True,
                 class_embed_type=None, addition_embed_type="text_time", addition_time_embed_dim=256, num_class_embeds=None,
                 upcast_attention=None, resnet_time_scale_shift="default", resnet_skip_time_act=False, resnet_out_scale_factor=1.0,
                 time_embedding_type="positional", time_embedding_dim=None, time_embedding_act_fn=None, timestep_post_act=None,
                 time_cond_proj_dim=None, conv_in_kernel=3, conv_out_kernel=3, projection_class_embeddings_input_dim=2816,
                 attention_type="default", class_embeddings_concat=False, mid_block_only_cross_attention=None, cross_attention_norm=None,
                 addition_embed_type_num_heads=64):
        super().__init__()
        given = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        self.config = Config(given)
        bad = []
        for k, want in _FIXED.items():
            ok = given[k] in want if isinstance(want, tuple) else given[k] == want
            if not ok:
                bad.append("%s=%r" % (k, given[k]))
        if bad:
            raise ValueError(_WHO + "unsupported configuration: " + ", ".join(bad) + " (the plan runs SDXL's values: "
                             + ", ".join("%s=%r" % (k, _FIXED[k]) for k in (b.split("=")[0] for b in bad)) + ")")
        heads = num_attention_heads or attention_head_dim        # diffusers' naming quirk: the head COUNT is read from attention_head_dim
        self._cfg = unet2d_config(in_channels, out_channels, down_block_types, up_block_types, block_out_channels, layers_per_block,
                                  transformer_layers_per_block, heads, cross_attention_dim, addition_time_embed_dim,
                                  projection_class_embeddings_input_dim, norm_eps)
        self._register_spec(unet2d_spec(self._cfg), dtype=torch.float32)
        # skip i of the down path: (channels, down-sampling factor), conv_in's output first
        n, boc, lpb = self._cfg.num_levels, list(self._cfg.block_out_channels), self._cfg.layers_per_block
        self._skips = [(boc[0], 1)]
        for i in range(n):
            self._skips += [(boc[i], 2 ** i)] * lpb + ([(boc[i], 2 ** (i + 1))] if i + 1 < n else [])
        self._mid = (boc[n - 1], 2 ** (n - 1))

    def config_dict(self):
        return {k: (list(v) if isinstance(v, tuple) else v) for k, v in self.config.items()}

    def _plan_created(self, slot):
        self._note_selection(L.lib().ctrl_unet2d_selection)

    def workspace_bytes(self):
        """bytes of the plan's forward workspace (the largest forward so far); 0 before the first forward"""
        return int(L.lib().ctrl_unet2d_workspace_bytes(self._plan)) if self._plan is not None else 0

    def _residual(self, r, what, B, h, w, chans, factor, dev):
        if not torch.is_tensor(r) or not r.is_cuda or r.device != dev:
            raise ValueError(_WHO + "%s must be a tensor on %s" % (what, dev))
        want = (B, chans, h // factor, w // factor)
        if tuple(r.shape) != want:
            raise ValueError(_WHO + "%s has shape %s, expected %s" % (what, tuple(r.shape), want))
        L.dtype_code(r.dtype)
        return r.contiguous()

    def _check_args(self, sample, encoder_hidden_states, class_labels, timestep_cond, attention_mask, cross_attention_kwargs,
                    added_cond_kwargs, mid_block_additional_residual, down_intrablock_additional_residuals, encoder_attention_mask):
        """the argument checks of forward that need no GPU: returns (text_embeds, time_ids, mid residual tensor or None)"""
        for name, v in (("class_labels", class_labels), ("timestep_cond", timestep_cond), ("attention_mask", attention_mask),
                        ("encoder_attention_mask", encoder_attention_mask),
                        ("down_intrablock_additional_residuals", down_intrablock_additional_residuals)):
            if v is not None:
                raise ValueError(_WHO + "`%s` is not supported by the plan (pass None)" % name)
        if cross_attention_kwargs:
            raise ValueError(_WHO + "`cross_attention_kwargs` must be empty (got keys %s)" % sorted(cross_attention_kwargs))
        if sample.dim() != 4 or sample.shape[1] != self._cfg.in_channels:
            raise ValueError(_WHO + "the sample must be [batch, %d, h, w] (got %s)" % (self._cfg.in_channels, tuple(sample.shape)))
        B, _, h, w = sample.shape
        if h % 8 or w % 8 or h < 8 or w < 8:
            raise ValueError(_WHO + "the latent height and width must be multiples of 8 (got %d x %d)" % (h, w))
        ehs, cross = encoder_hidden_states, self._cfg.cross_attention_dim
        if ehs.dim() != 3 or ehs.shape[0] != B or ehs.shape[2] != cross or ehs.shape[1] < 1:
            raise ValueError(_WHO + "encoder_hidden_states must be [%d, keys, %d] (got %s)" % (B, cross, tuple(ehs.shape)))
        if added_cond_kwargs is None:
            raise ValueError(_WHO + "addition_embed_type 'text_time' needs `added_cond_kwargs` with `text_embeds` and `time_ids`")
        extra = sorted(set(added_cond_kwargs) - {"text_embeds", "time_ids"})
        if extra:
            raise ValueError(_WHO + "unsupported key(s) %s in `added_cond_kwargs`: only `text_embeds` and `time_ids` run here "
                             "(no IP-Adapter `image_embeds`)" % extra)
        if "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
            raise ValueError(_WHO + "`added_cond_kwargs` must hold `text_embeds` and `time_ids`")
        text, ids = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
        if text.dim() != 2 or ids.dim() != 2 or text.shape[0] != B or ids.shape[0] != B:
            raise ValueError(_WHO + "text_embeds / time_ids must be [%d, n] (got %s / %s)" % (B, tuple(text.shape), tuple(ids.shape)))
        ad, pd = self._cfg.addition_time_embed_dim, self._cfg.projection_class_embeddings_input_dim
        if text.shape[1] + ids.shape[1] * ad != pd:
            raise ValueError(_WHO + "text_embeds.shape[1] + time_ids.shape[1] * addition_time_embed_dim = %d + %d * %d != "
                             "projection_class_embeddings_input_dim = %d" % (text.shape[1], ids.shape[1], ad, pd))
        mid = mid_block_additional_residual
        if mid is not None and not torch.is_tensor(mid):
            # the pipeline passes the Python number 0 when the adapter gives no mid residual
            if isinstance(mid, (int, float)) and not isinstance(mid, bool) and mid == 0:
                mid = None
            else:
                raise ValueError(_WHO + "`mid_block_additional_residual` must be a tensor, None or the number 0 (got %r)" % (mid,))
        return text, ids, mid

    @torch.no_grad()
    def forward(self, sample, timestep, encoder_hidden_states, class_labels=None, timestep_cond=None, attention_mask=None,
                cross_attention_kwargs=None, added_cond_kwargs=None, down_block_additional_residuals=None,
                mid_block_additional_residual=None, down_intrablock_additional_residuals=None, encoder_attention_mask=None,
                return_dict=True):
        text, ids, mid = self._check_args(sample, encoder_hidden_states, class_labels, timestep_cond, attention_mask, cross_attention_kwargs,
                                          added_cond_kwargs, mid_block_additional_residual, down_intrablock_additional_residuals,
                                          encoder_attention_mask)
        dev = _check_gpu_input(self, sample, "the sample")
        B, _, h, w = sample.shape
        sample = sample.contiguous()
        ehs = encoder_hidden_states.to(dev).contiguous()
        L.dtype_code(ehs.dtype)
        t = timesteps_to_device_f32(timestep, B, dev)
        text = text.to(dev).contiguous()
        ids = ids.detach().to(device=dev, dtype=torch.float32).contiguous()
        down, down_dt = [], L.F32
        if down_block_additional_residuals is not None and len(down_block_additional_residuals):
            # zip(): skip i takes residual i; the list may be shorter than the skips (the rest stay as they are), never longer
            res = list(down_block_additional_residuals)
            if len(res) > len(self._skips):
                raise ValueError(_WHO + "%d down_block_additional_residuals for %d skips" % (len(res), len(self._skips)))
            for i, r in enumerate(res):
                r = self._residual(r, "down_block_additional_residuals[%d]" % i, B, h, w, self._skips[i][0], self._skips[i][1], dev)
                down.append(r)
                if i == 0:
                    down_dt = L.dtype_code(r.dtype)
                elif L.dtype_code(r.dtype) != down_dt:
                    raise ValueError(_WHO + "down_block_additional_residuals must share one dtype")
        mid_dt = L.F32
        if mid is not None:
            mid = self._residual(mid, "mid_block_additional_residual", B, h, w, self._mid[0], self._mid[1], dev)
            mid_dt = L.dtype_code(mid.dtype)
        out = torch.empty((B, self._cfg.out_channels, h, w), dtype=sample.dtype, device=dev)
        ptrs = (C.c_void_p * max(len(down), 1))()
        for i, r in enumerate(down):
            ptrs[i] = r.data_ptr()
        with torch.cuda.device(dev):
            self._text_cache_mode(encoder_hidden_states, L.lib().ctrl_unet2d_set_text_cache)
            L.check(L.lib().ctrl_unet2d_forward(self._ensure_plan(), L.ptr(sample), L.dtype_code(sample.dtype), B, h, w, L.ptr(t), t.numel(),
                                                L.ptr(ehs), L.dtype_code(ehs.dtype), ehs.shape[1], L.ptr(text), L.dtype_code(text.dtype),
                                                text.shape[1], L.ptr(ids), ids.shape[1], ptrs, len(down), down_dt, L.ptr(mid), mid_dt,
                                                L.ptr(out), L.cur_stream()))
        L.raise_if_out_of_range(type(self).__name__)
        return UNet2DConditionOutput(out) if return_dict else (out,)
