"""fp32 PyTorch restatement of SDXL's backbone UNet: diffusers' UNet2DConditionModel in the configuration family SDXL-base uses
(addition_embed_type "text_time", use_linear_projection, a transformer depth per level).  Our own code, written from diffusers'
semantics; diffusers is not available here and the reference tree does not hold this class (it imports diffusers' at
sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py), so this restatement is NOT pinned against either --
tests/test_unet_sdxl_host.py holds its up blocks against oracle/blocks.py calls written out by hand instead.

Taken from oracle/blocks.py (imported read-only): ResnetBlock2D, DownBlock2D, Upsample2D, Downsample2D (inside the down blocks),
Timesteps, TimestepEmbedding, BasicTransformerBlock; Transformer2DModel, CrossAttnDownBlock2D and UNetMidBlock2DCrossAttn are the
oracle's classes too, subclassed for the two things the oracle's copies fix (they restate the SD-1.5 ControlNet): the projections
become nn.Linear on tokens (use_linear_projection; the oracle's are 1x1 convolutions, the same arithmetic with [C, C, 1, 1] keys) and
the transformer depth becomes an argument.  Restated here from their semantics: UpBlock2D, CrossAttnUpBlock2D, the text_time
embedding and the model.  Every ResNet takes norm_eps (1e-5), every transformer GroupNorm 1e-6, as diffusers builds them.  Same keys
and forward signature as ctrl_adapter_amd.UNet2DConditionModel."""
import torch
from torch import nn

import helpers  # noqa: F401  (puts the repository root on sys.path)
from oracle import blocks as O

_SDXL_TYPES = dict(down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                   up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"))
_TWO_TYPES = dict(down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"))
_SMALL = dict(cross_attention_dim=128, addition_time_embed_dim=32, projection_class_embeddings_input_dim=64 + 6 * 32, layers_per_block=2)

SDXL = dict(_SDXL_TYPES, block_out_channels=(320, 640, 1280), attention_head_dim=(5, 10, 20), transformer_layers_per_block=(1, 2, 10),
            cross_attention_dim=2048, addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816, layers_per_block=2)
TWO = dict(_TWO_TYPES, **_SMALL, block_out_channels=(64, 128), attention_head_dim=(1, 2), transformer_layers_per_block=(1, 2))
THREE = dict(_SDXL_TYPES, **_SMALL, block_out_channels=(64, 128, 256), attention_head_dim=(1, 2, 4), transformer_layers_per_block=(1, 2, 3))
LPB1 = dict(TWO, layers_per_block=1)
# real widths: K = 2048 (text K / V) and 2816 (add_embedding), the 960-channel join at 30 channels per group
WIDE = dict(_TWO_TYPES, block_out_channels=(320, 640), attention_head_dim=(5, 10), transformer_layers_per_block=(1, 1),
            cross_attention_dim=2048, addition_time_embed_dim=256, projection_class_embeddings_input_dim=1280 + 6 * 256, layers_per_block=2)
# a 1280 + 1280 concatenation (the real model's widest GroupNorm, 2560 channels: beyond the 2048 one GroupNorm launch covers)
CAT2560 = dict(_TWO_TYPES, **_SMALL, block_out_channels=(64, 1280), attention_head_dim=(1, 20), transformer_layers_per_block=(1, 1))
CONFIGS = {"TWO": TWO, "THREE": THREE, "LPB1": LPB1, "WIDE": WIDE, "CAT2560": CAT2560}


def text_dim(cfg):
    """width of text_embeds for six time ids (SDXL-base: original size, crop, target size)"""
    return cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]


class Transformer2DModel(O.Transformer2DModel):
    """the oracle's Transformer2DModel with use_linear_projection=True: proj_in / proj_out are nn.Linear applied to the tokens"""

    def __init__(self, num_attention_heads, attention_head_dim, in_channels, num_layers=1, cross_attention_dim=None):
        super().__init__(num_attention_heads, attention_head_dim, in_channels, num_layers, cross_attention_dim)
        inner = num_attention_heads * attention_head_dim
        self.proj_in = nn.Linear(in_channels, inner)
        self.proj_out = nn.Linear(inner, in_channels)

    def forward(self, hidden_states, encoder_hidden_states=None):
        b, _, h, w = hidden_states.shape
        residual = hidden_states
        x = self.norm(hidden_states)
        inner = x.shape[1]
        x = self.proj_in(x.permute(0, 2, 3, 1).reshape(b, h * w, inner))
        for blk in self.transformer_blocks:
            x = blk(x, encoder_hidden_states=encoder_hidden_states)
        x = self.proj_out(x)
        return x.reshape(b, h, w, inner).permute(0, 3, 1, 2).contiguous() + residual


def _transformers(n, channels, heads, depth, cross):
    return nn.ModuleList([Transformer2DModel(heads, channels // heads, channels, depth, cross) for _ in range(n)])


class CrossAttnDownBlock2D(O.CrossAttnDownBlock2D):
    def __init__(self, in_channels, out_channels, temb_channels, num_layers, resnet_eps, num_attention_heads, cross_attention_dim,
                 add_downsample, depth):
        super().__init__(in_channels, out_channels, temb_channels, num_layers, resnet_eps, num_attention_heads, cross_attention_dim,
                         add_downsample)
        self.attentions = _transformers(num_layers, out_channels, num_attention_heads, depth, cross_attention_dim)


class UNetMidBlock2DCrossAttn(O.UNetMidBlock2DCrossAttn):
    def __init__(self, in_channels, temb_channels, resnet_eps, num_attention_heads, cross_attention_dim, depth):
        super().__init__(in_channels, temb_channels, resnet_eps, num_attention_heads, cross_attention_dim)
        self.attentions = _transformers(1, in_channels, num_attention_heads, depth, cross_attention_dim)


class UpsampleConv(nn.Module):
    """diffusers Upsample2D(use_conv=True): the oracle's nearest x2, then a 3x3 convolution (key `conv`)"""

    def __init__(self, channels):
        super().__init__()
        self.up = O.Upsample2D(channels)
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)

    def forward(self, x):
        return self.conv(self.up(x))


class UpBlock2D(nn.Module):
    """diffusers UpBlock2D: per layer pop the last skip, concatenate [hidden | skip] along the channels, ResnetBlock2D; then Upsample2D.
    in_channels: the width of the skips the LAST layer meets (the level below), prev_output_channel: the incoming stream's"""
    has_cross_attention = False

    def __init__(self, in_channels, prev_output_channel, out_channels, temb_channels, num_layers, resnet_eps, add_upsample):
        super().__init__()
        self.resnets = nn.ModuleList()
        for i in range(num_layers):
            skip = in_channels if i == num_layers - 1 else out_channels
            cin = prev_output_channel if i == 0 else out_channels
            self.resnets.append(O.ResnetBlock2D(in_channels=cin + skip, out_channels=out_channels, temb_channels=temb_channels, eps=resnet_eps))
        self.upsamplers = nn.ModuleList([UpsampleConv(out_channels)]) if add_upsample else None

    def _layer(self, i, hidden_states, temb, encoder_hidden_states):
        return self.resnets[i](hidden_states, temb)

    def forward(self, hidden_states, res_hidden_states_tuple, temb=None, encoder_hidden_states=None):
        for i in range(len(self.resnets)):
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            hidden_states = self._layer(i, torch.cat([hidden_states, res], dim=1), temb, encoder_hidden_states)
        if self.upsamplers is not None:
            hidden_states = self.upsamplers[0](hidden_states)
        return hidden_states


class CrossAttnUpBlock2D(UpBlock2D):
    """diffusers CrossAttnUpBlock2D: UpBlock2D with a Transformer2DModel behind every ResNet"""
    has_cross_attention = True

    def __init__(self, in_channels, prev_output_channel, out_channels, temb_channels, num_layers, resnet_eps, add_upsample,
                 num_attention_heads, cross_attention_dim, depth):
        super().__init__(in_channels, prev_output_channel, out_channels, temb_channels, num_layers, resnet_eps, add_upsample)
        self.attentions = _transformers(num_layers, out_channels, num_attention_heads, depth, cross_attention_dim)

    def _layer(self, i, hidden_states, temb, encoder_hidden_states):
        return self.attentions[i](self.resnets[i](hidden_states, temb), encoder_hidden_states=encoder_hidden_states)


class _Out(tuple):
    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


class UNetSdxlRef(nn.Module):
    def __init__(self, sample_size=None, in_channels=4, out_channels=4, down_block_types=SDXL["down_block_types"],
                 up_block_types=SDXL["up_block_types"], block_out_channels=(320, 640, 1280), layers_per_block=2, norm_eps=1e-5,
                 cross_attention_dim=2048, transformer_layers_per_block=(1, 2, 10), attention_head_dim=(5, 10, 20), num_attention_heads=None,
                 addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816):
        super().__init__()
        boc, n = tuple(block_out_channels), len(block_out_channels)
        heads = num_attention_heads or attention_head_dim                   # diffusers' quirk: the head COUNT
        heads = (heads,) * n if isinstance(heads, int) else tuple(heads)
        depth = transformer_layers_per_block
        depth = (depth,) * n if isinstance(depth, int) else tuple(depth)
        lpb, cross, eps = layers_per_block, cross_attention_dim, norm_eps
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        temb = boc[0] * 4
        self.time_proj = O.Timesteps(boc[0], True, 0)
        self.time_embedding = O.TimestepEmbedding(boc[0], temb)
        self.add_time_proj = O.Timesteps(addition_time_embed_dim, True, 0)
        self.add_embedding = O.TimestepEmbedding(projection_class_embeddings_input_dim, temb)
        self.down_blocks = nn.ModuleList()
        out = boc[0]
        for i, kind in enumerate(down_block_types):
            cin, out, final = out, boc[i], i == n - 1
            if kind == "CrossAttnDownBlock2D":
                self.down_blocks.append(CrossAttnDownBlock2D(cin, out, temb, lpb, eps, heads[i], cross, not final, depth[i]))
            elif kind == "DownBlock2D":
                self.down_blocks.append(O.DownBlock2D(cin, out, temb, lpb, eps, not final))
            else:
                raise ValueError(kind)
        self.mid_block = UNetMidBlock2DCrossAttn(boc[-1], temb, eps, heads[-1], cross, depth[-1])
        self.up_blocks = nn.ModuleList()
        rev, rheads, rdepth = boc[::-1], heads[::-1], depth[::-1]           # the up path reads the REVERSED per-level lists
        out = rev[0]
        for i, kind in enumerate(up_block_types):
            prev, out, cin, final = out, rev[i], rev[min(i + 1, n - 1)], i == n - 1
            if kind == "CrossAttnUpBlock2D":
                self.up_blocks.append(CrossAttnUpBlock2D(cin, prev, out, temb, lpb + 1, eps, not final, rheads[i], cross, rdepth[i]))
            elif kind == "UpBlock2D":
                self.up_blocks.append(UpBlock2D(cin, prev, out, temb, lpb + 1, eps, not final))
            else:
                raise ValueError(kind)
        self.conv_norm_out = nn.GroupNorm(32, boc[0], eps=eps)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    def text_time_embedding(self, text_embeds, time_ids, dtype):
        """diffusers' `text_time` branch: add_time_proj(time_ids.flatten()) reshaped per sample, concat([text_embeds, time_embeds], -1)
        (text first), add_embedding"""
        time_embeds = self.add_time_proj(time_ids.flatten()).reshape((text_embeds.shape[0], -1))
        add_embeds = torch.concat([text_embeds, time_embeds.to(text_embeds.dtype)], dim=-1).to(dtype)
        return self.add_embedding(add_embeds)

    def forward(self, sample, timestep, encoder_hidden_states, class_labels=None, timestep_cond=None, attention_mask=None,
                cross_attention_kwargs=None, added_cond_kwargs=None, down_block_additional_residuals=None,
                mid_block_additional_residual=None, down_intrablock_additional_residuals=None, encoder_attention_mask=None,
                return_dict=True, return_stages=False):
        timesteps = timestep
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], dtype=torch.float64 if isinstance(timestep, float) else torch.int64, device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None].to(sample.device)
        timesteps = timesteps.expand(sample.shape[0])
        emb = self.time_embedding(self.time_proj(timesteps).to(sample.dtype))
        emb = emb + self.text_time_embedding(added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"], emb.dtype)
        sample = self.conv_in(sample)
        skips = (sample,)
        for blk in self.down_blocks:
            sample, res = blk(sample, temb=emb, encoder_hidden_states=encoder_hidden_states)
            skips += res
        if down_block_additional_residuals is not None:
            extra = list(down_block_additional_residuals)
            # skip i takes residual i; the skips a shorter list leaves unpaired stay as they are
            skips = tuple(s + r for s, r in zip(skips, extra)) + skips[len(extra):]
        all_skips = skips
        sample = self.mid_block(sample, temb=emb, encoder_hidden_states=encoder_hidden_states)
        if mid_block_additional_residual is not None:
            sample = sample + mid_block_additional_residual          # (the pipeline's Python 0 included)
        mid_out, ups = sample, []
        for blk in self.up_blocks:
            res = skips[-len(blk.resnets):]
            skips = skips[:-len(blk.resnets)]
            sample = blk(sample, res, temb=emb, encoder_hidden_states=encoder_hidden_states)
            ups.append(sample)
        sample = self.conv_out(self.conv_act(self.conv_norm_out(sample)))
        if return_stages:
            return sample, {"skips": all_skips, "mid": mid_out, "ups": ups}
        return _Out(sample) if return_dict else (sample,)


def seeded_unet(cfg, seed, cls=UNetSdxlRef):
    """cls(**cfg) with synthetic.seeded_init weights (unit gain, fp16-representable)"""
    from ctrl_adapter_amd.synthetic import seeded_init
    return seeded_init(cls(**cfg), seed=seed).eval()


@torch.no_grad()
def seeded_unet_on_device(cfg, seed, device, cls=UNetSdxlRef):
    """seeded_unet for models too large to draw on the CPU in a test's time: synthetic.seeded_init's distributions from ONE generator on
    the device -- >= 2-D weights N(0, 1 / fan_in), biases N(0, 0.1^2), norm scales 1 + N(0, 0.1^2), rounded to fp16-representable values"""
    with torch.device(device):
        m = cls(**cfg)
    g = torch.Generator(device=device).manual_seed(seed)
    for name, p in m.named_parameters():
        leaf = name.rsplit(".", 1)[-1]
        if p.dim() >= 2:
            v = torch.randn(p.shape, generator=g, device=p.device) / p[0].numel() ** 0.5
        elif leaf == "weight":
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        else:
            v = 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        p.copy_(v.half().float())
    return m.to(device).eval()


def skip_shapes(cfg, h, w):
    """[(channels, h, w)] of the skips in diffusers' order, and the mid block's"""
    boc, lpb = tuple(cfg["block_out_channels"]), cfg["layers_per_block"]
    out = [(boc[0], h, w)]
    for i, c in enumerate(boc):
        out += [(c, h >> i, w >> i)] * lpb
        if i + 1 < len(boc):
            out.append((c, h >> (i + 1), w >> (i + 1)))
    return out, (boc[-1], h >> (len(boc) - 1), w >> (len(boc) - 1))


def make_inputs(cfg, B, h, w, keys=77, seed=7, residuals=False, res_dtype=torch.float16, n_short=0, mid="tensor"):
    """fp16-representable inputs as the SDXL pipeline passes them: sample, timestep [B], encoder_hidden_states [B, keys, cross],
    added_cond_kwargs {text_embeds [B, text], time_ids [B, 6]}.  residuals: the down residuals (`n_short` fewer than the skips) in
    res_dtype, and the mid one as `mid` says: "tensor", None or 0"""
    from ctrl_adapter_amd.synthetic import seeded_tensor
    ids = torch.tensor([[512.0, 768.0, 0.0, 16.0, 512.0, 768.0]] * B) + 8.0 * torch.arange(B)[:, None].float()
    inp = dict(sample=seeded_tensor((B, cfg.get("in_channels", 4), h, w), seed),
               timestep=torch.tensor([37.0, 501.0, 12.0, 999.0][:B] if B <= 4 else [float(10 + 7 * i) for i in range(B)]),
               encoder_hidden_states=seeded_tensor((B, keys, cfg["cross_attention_dim"]), seed + 1),
               added_cond_kwargs=dict(text_embeds=seeded_tensor((B, text_dim(cfg)), seed + 2), time_ids=ids))
    if residuals:
        shapes, mid_shape = skip_shapes(cfg, h, w)
        inp["down_block_additional_residuals"] = [(0.5 * seeded_tensor((B,) + s, seed + 10 + i)).to(res_dtype)
                                                  for i, s in enumerate(shapes[:len(shapes) - n_short])]
        inp["mid_block_additional_residual"] = (0.5 * seeded_tensor((B,) + mid_shape, seed + 99)).to(res_dtype) if mid == "tensor" else mid
    return inp
