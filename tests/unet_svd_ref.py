"""fp32 PyTorch restatement of SVD's backbone UNet: diffusers v0.27.2's UNetSpatioTemporalConditionModel with the two ControlNet-residual
kwargs the reference adds (svd/models/unets/unet_spatio_temporal_condition.py: constructor :70-246, forward :357-526).  Our own code,
written from diffusers' semantics; diffusers is not available here, so this restatement is NOT pinned against it --
tests/test_unet_svd_host.py holds it against oracle/blocks.py instead: with the temporal branches switched off a restated
SpatioTemporalResBlock is the oracle's ResnetBlock2D bit for bit, a restated TransformerSpatioTemporalModel the oracle's
GroupNorm -> Linear -> BasicTransformerBlock -> Linear + input.

Built from oracle/blocks.py's classes (imported read-only): Timesteps, TimestepEmbedding, BasicTransformerBlock,
TemporalBasicTransformerBlock, ResnetBlock2D, TemporalResnetBlock, AlphaBlender, Upsample2D, Downsample2D.  Added here: what they lack --
SpatioTemporalResBlock with time embeddings, TransformerSpatioTemporalModel (with the reference's time-context pairing), the four
block types, the model.  ResNet eps follows diffusers' unet_3d_blocks.py: 1e-6 in the CrossAttnDown / both up blocks, 1e-5 in
DownBlockSpatioTemporal and the mid block.  Same keys and forward signature as ctrl_adapter_amd.UNetSpatioTemporalConditionModel."""
import torch
from torch import nn

import helpers  # noqa: F401  (puts the repository root on sys.path)
from oracle.blocks import (AlphaBlender, BasicTransformerBlock, Downsample2D, ResnetBlock2D, TemporalBasicTransformerBlock,
                           TemporalResnetBlock, TimestepEmbedding, Timesteps, Upsample2D)

MIX_CYCLE = (-1.5, 0.5, 2.0)

NARROW = dict(in_channels=8, out_channels=4, block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), layers_per_block=1,
              cross_attention_dim=64, addition_time_embed_dim=32, projection_class_embeddings_input_dim=96)
NARROW2 = dict(NARROW, layers_per_block=2)
WIDE2 = dict(in_channels=8, out_channels=4, block_out_channels=(320, 640), num_attention_heads=(5, 10), layers_per_block=1,
             cross_attention_dim=1024, addition_time_embed_dim=256, projection_class_embeddings_input_dim=768,
             down_block_types=("CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"),
             up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal"))
# a 1280 + 1280 concatenation (the real model's widest GroupNorm, 2560 channels: beyond the 2048 one GroupNorm launch covers) at two levels
CAT2560 = dict(NARROW, block_out_channels=(64, 1280), num_attention_heads=(1, 20),
               down_block_types=("CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"),
               up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal"))
CONFIGS = {"NARROW": NARROW, "NARROW2": NARROW2, "WIDE2": WIDE2}


class SpatioTemporalResBlock(nn.Module):
    """spatial ResnetBlock2D, then a TemporalResnetBlock over [B, C, F, H, W] with the per-frame embedding, then
    AlphaBlender(learned_with_images): alpha * spatial + (1 - alpha) * temporal"""

    def __init__(self, in_channels, out_channels, temb_channels, eps):
        super().__init__()
        self.spatial_res_block = ResnetBlock2D(in_channels=in_channels, out_channels=out_channels, temb_channels=temb_channels, eps=eps)
        self.temporal_res_block = TemporalResnetBlock(out_channels, out_channels, temb_channels=temb_channels, eps=eps)
        self.time_mixer = AlphaBlender(alpha=0.5, merge_strategy="learned_with_images", switch_spatial_to_temporal_mix=False)

    def forward(self, hidden_states, temb, image_only_indicator):
        num_frames = image_only_indicator.shape[-1]
        hidden_states = self.spatial_res_block(hidden_states, temb)
        bf, c, h, w = hidden_states.shape
        b = bf // num_frames
        mix = hidden_states[None, :].reshape(b, num_frames, c, h, w).permute(0, 2, 1, 3, 4)
        hidden_states = hidden_states[None, :].reshape(b, num_frames, c, h, w).permute(0, 2, 1, 3, 4)
        temb = temb.reshape(b, num_frames, -1)
        hidden_states = self.temporal_res_block(hidden_states, temb)
        hidden_states = self.time_mixer(x_spatial=mix, x_temporal=hidden_states, image_only_indicator=image_only_indicator)
        return hidden_states.permute(0, 2, 1, 3, 4).reshape(bf, c, h, w)


class TransformerSpatioTemporalModel(nn.Module):
    def __init__(self, num_attention_heads, attention_head_dim, in_channels, num_layers=1, cross_attention_dim=None):
        super().__init__()
        inner = num_attention_heads * attention_head_dim
        self.in_channels = in_channels
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6)
        self.proj_in = nn.Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, num_attention_heads, attention_head_dim, cross_attention_dim)
                                                 for _ in range(num_layers)])
        self.temporal_transformer_blocks = nn.ModuleList([
            TemporalBasicTransformerBlock(inner, inner, num_attention_heads, attention_head_dim, cross_attention_dim)
            for _ in range(num_layers)])
        self.time_pos_embed = TimestepEmbedding(in_channels, in_channels * 4, out_dim=in_channels)
        self.time_proj = Timesteps(in_channels, True, 0)
        self.time_mixer = AlphaBlender(alpha=0.5, merge_strategy="learned_with_images")
        self.proj_out = nn.Linear(inner, in_channels)

    def forward(self, hidden_states, encoder_hidden_states, image_only_indicator):
        bf, _, height, width = hidden_states.shape
        num_frames = image_only_indicator.shape[-1]
        batch = bf // num_frames
        # the first frame's context of every clip, broadcast over the pixels ORDERED (pixel, clip): the temporal block's rows are
        # (clip, pixel), so its row (b L + p) meets the context of clip (b L + p) % batch -- the reference's quirk, kept
        time_context = encoder_hidden_states
        first = time_context[None, :].reshape(batch, num_frames, -1, time_context.shape[-1])[:, 0]
        time_context = first[None, :].broadcast_to(height * width, batch, first.shape[-2], first.shape[-1])
        time_context = time_context.reshape(height * width * batch, first.shape[-2], first.shape[-1])
        residual = hidden_states
        hidden_states = self.norm(hidden_states)
        inner = hidden_states.shape[1]
        hidden_states = hidden_states.permute(0, 2, 3, 1).reshape(bf, height * width, inner)
        hidden_states = self.proj_in(hidden_states)
        frame_idx = torch.arange(num_frames, device=hidden_states.device).repeat(batch, 1).reshape(-1)
        emb = self.time_pos_embed(self.time_proj(frame_idx).to(hidden_states.dtype))[:, None, :]
        for block, temporal_block in zip(self.transformer_blocks, self.temporal_transformer_blocks):
            hidden_states = block(hidden_states, encoder_hidden_states=encoder_hidden_states)
            mix = hidden_states + emb
            mix = temporal_block(mix, num_frames=num_frames, encoder_hidden_states=time_context)
            hidden_states = self.time_mixer(x_spatial=hidden_states, x_temporal=mix, image_only_indicator=image_only_indicator)
        hidden_states = self.proj_out(hidden_states)
        hidden_states = hidden_states.reshape(bf, height, width, inner).permute(0, 3, 1, 2).contiguous()
        return hidden_states + residual


class UpsampleConv(nn.Module):
    """diffusers Upsample2D(use_conv=True): the oracle's nearest x2, then a 3x3 convolution (key `conv`)"""

    def __init__(self, channels):
        super().__init__()
        self.up = Upsample2D(channels)
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)

    def forward(self, x):
        return self.conv(self.up(x))


class _DownBlock(nn.Module):
    def __init__(self, cin, cout, temb, num_layers, add_downsample, eps, attn=None):
        super().__init__()
        self.has_cross_attention = attn is not None
        self.resnets = nn.ModuleList([SpatioTemporalResBlock(cin if i == 0 else cout, cout, temb, eps) for i in range(num_layers)])
        if attn is not None:
            heads, cross, tl = attn
            self.attentions = nn.ModuleList([TransformerSpatioTemporalModel(heads, cout // heads, cout, tl, cross) for _ in range(num_layers)])
        if add_downsample:
            self.downsamplers = nn.ModuleList([Downsample2D(cout, True, cout, 1, "op")])

    def forward(self, hidden_states, temb, encoder_hidden_states, image_only_indicator):
        outs = ()
        for i, resnet in enumerate(self.resnets):
            hidden_states = resnet(hidden_states, temb, image_only_indicator)
            if self.has_cross_attention:
                hidden_states = self.attentions[i](hidden_states, encoder_hidden_states, image_only_indicator)
            outs += (hidden_states,)
        if hasattr(self, "downsamplers"):
            hidden_states = self.downsamplers[0](hidden_states)
            outs += (hidden_states,)
        return hidden_states, outs


class CrossAttnDownBlockSpatioTemporal(_DownBlock):
    def __init__(self, cin, cout, temb, num_layers, heads, cross, tl, add_downsample):
        super().__init__(cin, cout, temb, num_layers, add_downsample, 1e-6, (heads, cross, tl))


class DownBlockSpatioTemporal(_DownBlock):
    def __init__(self, cin, cout, temb, num_layers, add_downsample):
        super().__init__(cin, cout, temb, num_layers, add_downsample, 1e-5)


class UNetMidBlockSpatioTemporal(nn.Module):
    def __init__(self, channels, temb, heads, cross, tl):
        super().__init__()
        self.resnets = nn.ModuleList([SpatioTemporalResBlock(channels, channels, temb, 1e-5) for _ in range(2)])
        self.attentions = nn.ModuleList([TransformerSpatioTemporalModel(heads, channels // heads, channels, tl, cross)])

    def forward(self, hidden_states, temb, encoder_hidden_states, image_only_indicator):
        hidden_states = self.resnets[0](hidden_states, temb, image_only_indicator)
        for attn, resnet in zip(self.attentions, self.resnets[1:]):
            hidden_states = attn(hidden_states, encoder_hidden_states, image_only_indicator)
            hidden_states = resnet(hidden_states, temb, image_only_indicator)
        return hidden_states


class _UpBlock(nn.Module):
    def __init__(self, cin, prev, cout, temb, num_layers, add_upsample, attn=None):
        super().__init__()
        self.has_cross_attention = attn is not None
        self.resnets = nn.ModuleList()
        for i in range(num_layers):
            skip = cin if i == num_layers - 1 else cout
            self.resnets.append(SpatioTemporalResBlock((prev if i == 0 else cout) + skip, cout, temb, 1e-6))
        if attn is not None:
            heads, cross, tl = attn
            self.attentions = nn.ModuleList([TransformerSpatioTemporalModel(heads, cout // heads, cout, tl, cross) for _ in range(num_layers)])
        if add_upsample:
            self.upsamplers = nn.ModuleList([UpsampleConv(cout)])

    def forward(self, hidden_states, res_hidden_states_tuple, temb, encoder_hidden_states, image_only_indicator):
        for i, resnet in enumerate(self.resnets):
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            hidden_states = torch.cat([hidden_states, res], dim=1)
            hidden_states = resnet(hidden_states, temb, image_only_indicator)
            if self.has_cross_attention:
                hidden_states = self.attentions[i](hidden_states, encoder_hidden_states, image_only_indicator)
        if hasattr(self, "upsamplers"):
            hidden_states = self.upsamplers[0](hidden_states)
        return hidden_states


class UpBlockSpatioTemporal(_UpBlock):
    def __init__(self, cin, prev, cout, temb, num_layers, add_upsample):
        super().__init__(cin, prev, cout, temb, num_layers, add_upsample)


class CrossAttnUpBlockSpatioTemporal(_UpBlock):
    def __init__(self, cin, prev, cout, temb, num_layers, heads, cross, tl, add_upsample):
        super().__init__(cin, prev, cout, temb, num_layers, add_upsample, (heads, cross, tl))


class _Out(tuple):
    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


class UNetSvdRef(nn.Module):
    def __init__(self, sample_size=None, in_channels=8, out_channels=4,
                 down_block_types=("CrossAttnDownBlockSpatioTemporal", "CrossAttnDownBlockSpatioTemporal",
                                   "CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"),
                 up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal",
                                 "CrossAttnUpBlockSpatioTemporal"),
                 block_out_channels=(320, 640, 1280, 1280), addition_time_embed_dim=256, projection_class_embeddings_input_dim=768,
                 layers_per_block=2, cross_attention_dim=1024, transformer_layers_per_block=1, num_attention_heads=(5, 10, 10, 20),
                 num_frames=25):
        super().__init__()
        boc, n = tuple(block_out_channels), len(block_out_channels)
        heads = (num_attention_heads,) * n if isinstance(num_attention_heads, int) else tuple(num_attention_heads)
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        temb = boc[0] * 4
        self.time_proj = Timesteps(boc[0], True, 0)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        self.add_time_proj = Timesteps(addition_time_embed_dim, True, 0)
        self.add_embedding = TimestepEmbedding(projection_class_embeddings_input_dim, temb)
        lpb, cross, tl = layers_per_block, cross_attention_dim, transformer_layers_per_block
        self.down_blocks = nn.ModuleList()
        out = boc[0]
        for i, kind in enumerate(down_block_types):
            cin, out, final = out, boc[i], i == n - 1
            if kind == "CrossAttnDownBlockSpatioTemporal":
                self.down_blocks.append(CrossAttnDownBlockSpatioTemporal(cin, out, temb, lpb, heads[i], cross, tl, not final))
            elif kind == "DownBlockSpatioTemporal":
                self.down_blocks.append(DownBlockSpatioTemporal(cin, out, temb, lpb, not final))
            else:
                raise ValueError(kind)
        self.mid_block = UNetMidBlockSpatioTemporal(boc[-1], temb, heads[-1], cross, tl)
        self.up_blocks = nn.ModuleList()
        rev, rheads = boc[::-1], heads[::-1]
        out = rev[0]
        for i, kind in enumerate(up_block_types):
            prev, out, cin, final = out, rev[i], rev[min(i + 1, n - 1)], i == n - 1
            if kind == "CrossAttnUpBlockSpatioTemporal":
                self.up_blocks.append(CrossAttnUpBlockSpatioTemporal(cin, prev, out, temb, lpb + 1, rheads[i], cross, tl, not final))
            elif kind == "UpBlockSpatioTemporal":
                self.up_blocks.append(UpBlockSpatioTemporal(cin, prev, out, temb, lpb + 1, not final))
            else:
                raise ValueError(kind)
        self.conv_norm_out = nn.GroupNorm(32, boc[0], eps=1e-5)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    def forward(self, sample, timestep, encoder_hidden_states, added_time_ids, down_block_additional_residuals=None,
                mid_block_additional_residual=None, return_dict=True, return_stages=False):
        timesteps = timestep
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], dtype=torch.float64 if isinstance(timestep, float) else torch.int64, device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None].to(sample.device)
        batch, num_frames = sample.shape[:2]
        timesteps = timesteps.expand(batch)
        emb = self.time_embedding(self.time_proj(timesteps).to(sample.dtype))
        time_embeds = self.add_time_proj(added_time_ids.flatten()).reshape((batch, -1)).to(emb.dtype)
        emb = emb + self.add_embedding(time_embeds)
        sample = sample.flatten(0, 1)
        emb = emb.repeat_interleave(num_frames, dim=0)
        encoder_hidden_states = encoder_hidden_states.repeat_interleave(num_frames, dim=0)
        sample = self.conv_in(sample)
        ioi = torch.zeros(batch, num_frames, dtype=sample.dtype, device=sample.device)
        skips = (sample,)
        for blk in self.down_blocks:
            sample, res = blk(sample, emb, encoder_hidden_states, ioi)
            skips += res
        if down_block_additional_residuals is not None:
            extra = list(down_block_additional_residuals)
            if extra and extra[0].dim() == 5:
                extra = [r.permute(0, 2, 1, 3, 4).flatten(0, 1) for r in extra]          # b c f h w -> (b f) c h w
            # zip(): skip i takes residual i.  (The reference also DROPS the skips a shorter list leaves unpaired, after which its up
            # path cannot run; here they stay as they are -- the only reading under which a shorter list computes anything.)
            skips = tuple(s + r for s, r in zip(skips, extra)) + skips[len(extra):]
        all_skips = skips
        sample = self.mid_block(sample, emb, encoder_hidden_states, ioi)
        if mid_block_additional_residual is not None:
            r = mid_block_additional_residual
            if r.dim() == 5:
                r = r.permute(0, 2, 1, 3, 4).flatten(0, 1)
            sample = sample + r
        mid_out, ups = sample, []
        for blk in self.up_blocks:
            res = skips[-len(blk.resnets):]
            skips = skips[:-len(blk.resnets)]
            sample = blk(sample, res, emb, encoder_hidden_states, ioi)
            ups.append(sample)
        sample = self.conv_out(self.conv_act(self.conv_norm_out(sample)))
        sample = sample.reshape(batch, num_frames, *sample.shape[1:])
        if return_stages:
            return sample, {"skips": all_skips, "mid": mid_out, "ups": ups}
        return _Out(sample) if return_dict else (sample,)


@torch.no_grad()
def set_distinct_mix_factors(module):
    """after seeded_init (every mix_factor 0.5): values cycling through -1.5, 0.5 and 2.0 in state-dict order, so that a swapped blend
    or a mixer read from another block is an O(0.1) error"""
    i = 0
    for name, p in module.named_parameters():
        if name.endswith("mix_factor"):
            p.fill_(MIX_CYCLE[i % len(MIX_CYCLE)])
            i += 1
    assert i > 0
    return module


def seeded_unet(cfg, seed, cls=UNetSvdRef):
    """cls(**cfg) with synthetic.seeded_init weights and distinct mix factors"""
    from ctrl_adapter_amd.synthetic import seeded_init
    return set_distinct_mix_factors(seeded_init(cls(**cfg), seed=seed)).eval()


@torch.no_grad()
def seeded_unet_on_device(cfg, seed, device, cls=UNetSvdRef):
    """seeded_unet for models too large to draw on the CPU in a test's time (0.3 .. 1.5 G parameters): synthetic.seeded_init's
    distributions from ONE generator on the device -- >= 2-D weights N(0, 1 / fan_in), biases N(0, 0.1^2), norm scales 1 + N(0, 0.1^2),
    rounded to fp16-representable values -- and the distinct mix factors"""
    with torch.device(device):
        m = cls(**cfg)
    g = torch.Generator(device=device).manual_seed(seed)
    for name, p in m.named_parameters():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "mix_factor":
            continue
        if p.dim() >= 2:
            v = torch.randn(p.shape, generator=g, device=p.device) / p[0].numel() ** 0.5
        elif leaf == "weight":
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        else:
            v = 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        p.copy_(v.half().float())
    return set_distinct_mix_factors(m).to(device).eval()


def skip_shapes(cfg, B, F, h, w):
    """[(channels, h, w)] of the skips in the reference's order, and the mid block's"""
    boc, lpb = tuple(cfg["block_out_channels"]), cfg["layers_per_block"]
    out = [(boc[0], h, w)]
    for i, c in enumerate(boc):
        out += [(c, h >> i, w >> i)] * lpb
        if i + 1 < len(boc):
            out.append((c, h >> (i + 1), w >> (i + 1)))
    return out, (boc[-1], h >> (len(boc) - 1), w >> (len(boc) - 1))


def seeded_inputs(cfg, B, F, h, w, seed=7, residuals=None, res_dtype=torch.float16):
    """fp16-representable inputs: sample, timestep [B], encoder_hidden_states [B, 1, cross], added_time_ids [B, n]; residuals: None,
    "4d" ((b f) c h w) or "5d" (b c f h w) -> the twelve (or fewer) down residuals and the mid one, in res_dtype"""
    from ctrl_adapter_amd.synthetic import seeded_tensor
    n_ids = cfg["projection_class_embeddings_input_dim"] // cfg["addition_time_embed_dim"]
    inp = dict(sample=seeded_tensor((B, F, cfg["in_channels"], h, w), seed),
               timestep=torch.tensor([37.0, 501.0, 12.0, 999.0][:B] if B <= 4 else [float(10 + 7 * i) for i in range(B)]),
               encoder_hidden_states=seeded_tensor((B, 1, cfg["cross_attention_dim"]), seed + 1),
               added_time_ids=torch.tensor([[6.0, 127.0, 0.02]] * B)[:, :n_ids] + torch.arange(B)[:, None].float())
    if residuals:
        shapes, mid = skip_shapes(cfg, B, F, h, w)

        def one(i, c, hh, ww):
            t = 0.5 * seeded_tensor((B * F, c, hh, ww), seed + 10 + i)
            if residuals == "5d":
                t = t.reshape(B, F, c, hh, ww).permute(0, 2, 1, 3, 4).contiguous()
            return t.to(res_dtype)
        inp["down_block_additional_residuals"] = [one(i, *s) for i, s in enumerate(shapes)]
        inp["mid_block_additional_residual"] = one(99, *mid)
    return inp
