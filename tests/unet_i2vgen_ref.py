"""fp32 PyTorch restatement of I2VGen-XL's backbone UNet: I2VGenXLUNet as the reference extends it with the two ControlNet-residual
kwargs (i2vgen_xl/models/unets/unet_i2vgen_xl.py: constructor :134-322, forward :519-761, the residual additions :681-714).  Our own
code.  The 3D blocks, TemporalConvLayer and TransformerTemporalModel the reference imports are written from diffusers v0.27's
semantics; diffusers is not available here, so this restatement is NOT pinned against it --
tests/test_unet_i2vgen_host.py holds TemporalConvLayerRef and TransformerTemporalRef against the same arithmetic written out with
plain F.group_norm / F.conv3d / F.scaled_dot_product_attention instead.

Built from oracle/blocks.py's classes (imported read-only): Timesteps, TimestepEmbedding, Attention, BasicTransformerBlock,
ResnetBlock2D, Upsample2D, Downsample2D.  Added here: TemporalConvLayerRef (four GroupNorm + SiLU + (3,1,1) convolutions over
b c f h w, plus the identity), TransformerTemporalRef (GroupNorm over the clip, Linear, one BasicTransformerBlock whose two attentions
both run over the frames of a pixel, Linear, plus the input), Transformer2DLinear (diffusers' Transformer2DModel with linear
projections), LatentTemporalEncoderRef (I2VGenXLTransformerTemporalEncoder), the four block types and the model.  Same keys and forward
signature as ctrl_adapter_amd.I2VGenXLUNet."""
import torch
import torch.nn.functional as F
from torch import nn

import helpers  # noqa: F401  (puts the repository root on sys.path)
from oracle.blocks import Attention, BasicTransformerBlock, Downsample2D, ResnetBlock2D, TimestepEmbedding, Timesteps, Upsample2D

_D2 = ("CrossAttnDownBlock3D", "DownBlock3D")
_U2 = ("UpBlock3D", "CrossAttnUpBlock3D")
NARROW = dict(in_channels=4, out_channels=4, block_out_channels=(64, 128), down_block_types=_D2, up_block_types=_U2, layers_per_block=1,
              cross_attention_dim=128)
THREE = dict(in_channels=4, out_channels=4, block_out_channels=(64, 128, 128),
             down_block_types=("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
             up_block_types=("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"), layers_per_block=2, cross_attention_dim=128)
WIDE2 = dict(NARROW, block_out_channels=(320, 640), cross_attention_dim=1024)
# a 1280 + 1280 concatenation (the real model's widest GroupNorm, 2560 channels) at two levels; drawn on the device
CAT2560 = dict(NARROW, block_out_channels=(1280, 1280), cross_attention_dim=1024)
# the real config; used on the meta device only
I2VGEN = dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
              down_block_types=("CrossAttnDownBlock3D",) * 3 + ("DownBlock3D",), up_block_types=("UpBlock3D",) + ("CrossAttnUpBlock3D",) * 3,
              layers_per_block=2, cross_attention_dim=1024)
CONFIGS = {"NARROW": NARROW, "THREE": THREE, "WIDE2": WIDE2, "CAT2560": CAT2560, "I2VGEN": I2VGEN}
LATENT_TOKENS = 64           # AdaptiveAvgPool2d((32, 32)) and two stride-2 convolutions: 8 x 8


def _to_5d(x, num_frames):
    bf, c, h, w = x.shape
    return x[None, :].reshape(bf // num_frames, num_frames, c, h, w).permute(0, 2, 1, 3, 4)


def _to_4d(x):
    b, c, f, h, w = x.shape
    return x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)


class TemporalConvLayerRef(nn.Module):
    """diffusers TemporalConvLayer(dim, dim, norm_num_groups=32): identity + conv4(conv3(conv2(conv1(x)))) over b c f h w"""

    def __init__(self, dim):
        super().__init__()
        self.conv1 = nn.Sequential(nn.GroupNorm(32, dim), nn.SiLU(), nn.Conv3d(dim, dim, (3, 1, 1), padding=(1, 0, 0)))
        for i in (2, 3, 4):
            setattr(self, "conv%d" % i, nn.Sequential(nn.GroupNorm(32, dim), nn.SiLU(), nn.Dropout(0.0),
                                                       nn.Conv3d(dim, dim, (3, 1, 1), padding=(1, 0, 0))))

    def forward(self, hidden_states, num_frames=1):
        x = _to_5d(hidden_states, num_frames)
        x = x + self.conv4(self.conv3(self.conv2(self.conv1(x))))
        return _to_4d(x)


class TransformerTemporalRef(nn.Module):
    """diffusers TransformerTemporalModel(heads, head_dim, in_channels, num_layers=1, norm_num_groups=32): double_self_attention"""

    def __init__(self, num_attention_heads, attention_head_dim, in_channels):
        super().__init__()
        inner = num_attention_heads * attention_head_dim
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6)
        self.proj_in = nn.Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, num_attention_heads, attention_head_dim, None)])
        self.proj_out = nn.Linear(inner, in_channels)

    def forward(self, hidden_states, num_frames=1):
        bf, c, h, w = hidden_states.shape
        b = bf // num_frames
        x = self.norm(_to_5d(hidden_states, num_frames))                            # statistics over the clip
        x = x.permute(0, 3, 4, 2, 1).reshape(b * h * w, num_frames, c)              # (b h w, f, c)
        x = self.proj_in(x)
        for blk in self.transformer_blocks:
            x = blk(x, encoder_hidden_states=None)                                  # attn2 attends over the frames too
        x = self.proj_out(x)
        x = x[None, None, :].reshape(b, h, w, num_frames, c).permute(0, 3, 4, 1, 2).reshape(bf, c, h, w)
        return x + hidden_states


class Transformer2DLinear(nn.Module):
    """diffusers Transformer2DModel(use_linear_projection=True), one layer"""

    def __init__(self, num_attention_heads, attention_head_dim, in_channels, cross_attention_dim):
        super().__init__()
        inner = num_attention_heads * attention_head_dim
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6)
        self.proj_in = nn.Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, num_attention_heads, attention_head_dim, cross_attention_dim)])
        self.proj_out = nn.Linear(inner, in_channels)

    def forward(self, hidden_states, encoder_hidden_states=None):
        b, c, h, w = hidden_states.shape
        x = self.norm(hidden_states).permute(0, 2, 3, 1).reshape(b, h * w, c)
        x = self.proj_in(x)
        for blk in self.transformer_blocks:
            x = blk(x, encoder_hidden_states=encoder_hidden_states)
        x = self.proj_out(x)
        return x.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous() + hidden_states


class _GeluProj(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out)

    def forward(self, x):
        return F.gelu(self.proj(x))          # exact (erf)


class _FeedForwardGelu(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.net = nn.ModuleList([_GeluProj(dim, inner), nn.Dropout(0.0), nn.Linear(inner, dim)])

    def forward(self, x):
        for m in self.net:
            x = m(x)
        return x


class LatentTemporalEncoderRef(nn.Module):
    """I2VGenXLTransformerTemporalEncoder (unet_i2vgen_xl.py:55-101): LayerNorm, self-attention over the frames, feed-forward (gelu)"""

    def __init__(self, dim, num_attention_heads, attention_head_dim, ff_inner_dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-5)
        self.attn1 = Attention(dim, None, num_attention_heads, attention_head_dim, bias=False, out_bias=True)
        self.ff = _FeedForwardGelu(dim, ff_inner_dim)

    def forward(self, hidden_states):
        hidden_states = self.attn1(self.norm1(hidden_states)) + hidden_states
        return self.ff(hidden_states) + hidden_states


class UpsampleConv(nn.Module):
    """diffusers Upsample2D(use_conv=True): the oracle's nearest x2, then a 3x3 convolution (key `conv`)"""

    def __init__(self, channels):
        super().__init__()
        self.up = Upsample2D(channels)
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)

    def forward(self, x):
        return self.conv(self.up(x))


class _Layers(nn.Module):
    def _build(self, cins, cout, temb, cross):
        self.has_cross_attention = cross is not None
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels=c, out_channels=cout, temb_channels=temb, eps=1e-5) for c in cins])
        self.temp_convs = nn.ModuleList([TemporalConvLayerRef(cout) for _ in cins])
        if cross is not None:
            self.attentions = nn.ModuleList([Transformer2DLinear(cout // 64, 64, cout, cross) for _ in cins])
            self.temp_attentions = nn.ModuleList([TransformerTemporalRef(cout // 64, 64, cout) for _ in cins])

    def _layer(self, i, x, temb, ctx, num_frames):
        x = self.temp_convs[i](self.resnets[i](x, temb), num_frames=num_frames)
        if self.has_cross_attention:
            x = self.temp_attentions[i](self.attentions[i](x, encoder_hidden_states=ctx), num_frames=num_frames)
        return x


class _DownBlock3D(_Layers):
    def __init__(self, cin, cout, temb, num_layers, add_downsample, cross=None):
        super().__init__()
        self._build([cin if i == 0 else cout for i in range(num_layers)], cout, temb, cross)
        if add_downsample:
            self.downsamplers = nn.ModuleList([Downsample2D(cout, True, cout, 1, "op")])

    def forward(self, hidden_states, temb, ctx, num_frames):
        outs = ()
        for i in range(len(self.resnets)):
            hidden_states = self._layer(i, hidden_states, temb, ctx, num_frames)
            outs += (hidden_states,)
        if hasattr(self, "downsamplers"):
            hidden_states = self.downsamplers[0](hidden_states)
            outs += (hidden_states,)
        return hidden_states, outs


class CrossAttnDownBlock3D(_DownBlock3D):
    def __init__(self, cin, cout, temb, num_layers, cross, add_downsample):
        super().__init__(cin, cout, temb, num_layers, add_downsample, cross)


class DownBlock3D(_DownBlock3D):
    def __init__(self, cin, cout, temb, num_layers, add_downsample):
        super().__init__(cin, cout, temb, num_layers, add_downsample)


class UNetMidBlock3DCrossAttn(nn.Module):
    """resnets.0, temp_convs.0, then attentions.0, temp_attentions.0, resnets.1, temp_convs.1"""

    def __init__(self, channels, temb, cross):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels=channels, out_channels=channels, temb_channels=temb, eps=1e-5) for _ in range(2)])
        self.temp_convs = nn.ModuleList([TemporalConvLayerRef(channels) for _ in range(2)])
        self.attentions = nn.ModuleList([Transformer2DLinear(channels // 64, 64, channels, cross)])
        self.temp_attentions = nn.ModuleList([TransformerTemporalRef(channels // 64, 64, channels)])

    def forward(self, hidden_states, temb, ctx, num_frames):
        hidden_states = self.temp_convs[0](self.resnets[0](hidden_states, temb), num_frames=num_frames)
        hidden_states = self.temp_attentions[0](self.attentions[0](hidden_states, encoder_hidden_states=ctx), num_frames=num_frames)
        return self.temp_convs[1](self.resnets[1](hidden_states, temb), num_frames=num_frames)


class _UpBlock3D(_Layers):
    def __init__(self, cin, prev, cout, temb, num_layers, add_upsample, cross=None):
        super().__init__()
        self._build([(prev if i == 0 else cout) + (cin if i == num_layers - 1 else cout) for i in range(num_layers)], cout, temb, cross)
        if add_upsample:
            self.upsamplers = nn.ModuleList([UpsampleConv(cout)])

    def forward(self, hidden_states, res_hidden_states_tuple, temb, ctx, num_frames):
        for i in range(len(self.resnets)):
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            hidden_states = self._layer(i, torch.cat([hidden_states, res], dim=1), temb, ctx, num_frames)
        if hasattr(self, "upsamplers"):
            hidden_states = self.upsamplers[0](hidden_states)
        return hidden_states


class UpBlock3D(_UpBlock3D):
    def __init__(self, cin, prev, cout, temb, num_layers, add_upsample):
        super().__init__(cin, prev, cout, temb, num_layers, add_upsample)


class CrossAttnUpBlock3D(_UpBlock3D):
    def __init__(self, cin, prev, cout, temb, num_layers, cross, add_upsample):
        super().__init__(cin, prev, cout, temb, num_layers, add_upsample, cross)


class _Out(tuple):
    def __new__(cls, sample):
        self = super().__new__(cls, (sample,))
        self.sample = sample
        return self


class I2VGenUNetRef(nn.Module):
    def __init__(self, sample_size=None, in_channels=4, out_channels=4,
                 down_block_types=("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
                 up_block_types=("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"),
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, norm_num_groups=32, cross_attention_dim=1024,
                 attention_head_dim=64, num_attention_heads=None):
        super().__init__()
        assert norm_num_groups == 32 and attention_head_dim == 64
        boc, n, cross, lpb = tuple(block_out_channels), len(block_out_channels), cross_attention_dim, layers_per_block
        self.in_channels, self.cross_attention_dim = in_channels, cross
        self.conv_in = nn.Conv2d(in_channels + in_channels, boc[0], 3, padding=1)
        self.transformer_in = TransformerTemporalRef(8, 64, boc[0])
        self.image_latents_proj_in = nn.Sequential(nn.Conv2d(4, in_channels * 4, 3, padding=1), nn.SiLU(),
                                                   nn.Conv2d(in_channels * 4, in_channels * 4, 3, stride=1, padding=1), nn.SiLU(),
                                                   nn.Conv2d(in_channels * 4, in_channels, 3, stride=1, padding=1))
        self.image_latents_temporal_encoder = LatentTemporalEncoderRef(in_channels, 2, in_channels, in_channels * 4)
        self.image_latents_context_embedding = nn.Sequential(nn.Conv2d(4, in_channels * 8, 3, padding=1), nn.SiLU(), nn.AdaptiveAvgPool2d((32, 32)),
                                                             nn.Conv2d(in_channels * 8, in_channels * 16, 3, stride=2, padding=1), nn.SiLU(),
                                                             nn.Conv2d(in_channels * 16, cross, 3, stride=2, padding=1))
        temb = boc[0] * 4
        self.time_proj = Timesteps(boc[0], True, 0)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        self.context_embedding = nn.Sequential(nn.Linear(cross, temb), nn.SiLU(), nn.Linear(temb, cross * in_channels))
        self.fps_embedding = nn.Sequential(nn.Linear(boc[0], temb), nn.SiLU(), nn.Linear(temb, temb))
        self.down_blocks = nn.ModuleList()
        out = boc[0]
        for i, kind in enumerate(down_block_types):
            cin, out, final = out, boc[i], i == n - 1
            if kind == "CrossAttnDownBlock3D":
                self.down_blocks.append(CrossAttnDownBlock3D(cin, out, temb, lpb, cross, not final))
            elif kind == "DownBlock3D":
                self.down_blocks.append(DownBlock3D(cin, out, temb, lpb, not final))
            else:
                raise ValueError(kind)
        self.mid_block = UNetMidBlock3DCrossAttn(boc[-1], temb, cross)
        self.up_blocks = nn.ModuleList()
        rev = boc[::-1]
        out = rev[0]
        for i, kind in enumerate(up_block_types):
            prev, out, cin, final = out, rev[i], rev[min(i + 1, n - 1)], i == n - 1
            if kind == "CrossAttnUpBlock3D":
                self.up_blocks.append(CrossAttnUpBlock3D(cin, prev, out, temb, lpb + 1, cross, not final))
            elif kind == "UpBlock3D":
                self.up_blocks.append(UpBlock3D(cin, prev, out, temb, lpb + 1, not final))
            else:
                raise ValueError(kind)
        self.conv_norm_out = nn.GroupNorm(32, boc[0], eps=1e-5)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    def forward(self, sample, timestep, fps, image_latents, image_embeddings=None, encoder_hidden_states=None, timestep_cond=None,
                cross_attention_kwargs=None, down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict=True,
                return_stages=False):
        batch, channels, num_frames, height, width = sample.shape
        timesteps = timestep
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], dtype=torch.float64 if isinstance(timestep, float) else torch.int64, device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None].to(sample.device)
        timesteps = timesteps.expand(batch)
        t_emb = self.time_embedding(self.time_proj(timesteps).to(self.dtype))
        fps = fps.expand(fps.shape[0])
        fps_emb = self.fps_embedding(self.time_proj(fps).to(self.dtype))
        emb = (t_emb + fps_emb).repeat_interleave(num_frames, dim=0)
        # the context: text tokens | the first frame's latents as 64 tokens | the image embedding as in_channels tokens
        first = image_latents[:, :, :1]
        first = first.permute(0, 2, 1, 3, 4).reshape(batch, first.shape[1], height, width)
        lat_ctx = self.image_latents_context_embedding(first)
        lat_ctx = lat_ctx.permute(0, 2, 3, 1).reshape(batch, -1, lat_ctx.shape[1])
        image_emb = self.context_embedding(image_embeddings).view(-1, self.in_channels, self.cross_attention_dim)
        context = torch.cat([encoder_hidden_states, lat_ctx, image_emb], dim=1).repeat_interleave(num_frames, dim=0)
        # the image latents: proj_in per frame, the temporal encoder per pixel
        lat = self.image_latents_proj_in(_to_4d(image_latents))
        lat = lat[None, :].reshape(batch, num_frames, channels, height, width).permute(0, 3, 4, 1, 2)
        lat = self.image_latents_temporal_encoder(lat.reshape(batch * height * width, num_frames, channels))
        lat = lat.reshape(batch, height, width, num_frames, channels).permute(0, 4, 3, 1, 2)
        sample = _to_4d(torch.cat([sample, lat], dim=1))
        sample = self.conv_in(sample)
        sample = self.transformer_in(sample, num_frames=num_frames)
        skips = (sample,)
        for blk in self.down_blocks:
            sample, res = blk(sample, emb, context, num_frames)
            skips += res
        if down_block_additional_residuals is not None:
            extra = list(down_block_additional_residuals)
            if extra and extra[0].dim() == 5:
                extra = [_to_4d(r) for r in extra]                                  # b c f h w -> (b f) c h w
            # zip(): skip i takes residual i (a shorter list leaves the rest as they are, as in tests/unet_svd_ref.py)
            skips = tuple(s + r for s, r in zip(skips, extra)) + skips[len(extra):]
        all_skips = skips
        sample = self.mid_block(sample, emb, context, num_frames)
        if mid_block_additional_residual is not None:
            r = mid_block_additional_residual
            sample = sample + (_to_4d(r) if r.dim() == 5 else r)
        mid_out = sample
        for blk in self.up_blocks:
            res = skips[-len(blk.resnets):]
            skips = skips[:-len(blk.resnets)]
            sample = blk(sample, res, emb, context, num_frames)
        sample = self.conv_out(self.conv_act(self.conv_norm_out(sample)))
        sample = sample[None, :].reshape((-1, num_frames) + sample.shape[1:]).permute(0, 2, 1, 3, 4)
        if return_stages:
            return sample, {"skips": all_skips, "mid": mid_out}
        return _Out(sample) if return_dict else (sample,)


def seeded_unet(cfg, seed, cls=I2VGenUNetRef):
    """cls(**cfg) with synthetic.seeded_init weights: every >= 2-D weight N(0, 1 / fan_in) -- the convolutions diffusers initialises to
    zero (conv4 of every TemporalConvLayer, the transformers' proj_out) included, so the temporal path carries signal"""
    from ctrl_adapter_amd.synthetic import seeded_init
    m = seeded_init(cls(**cfg), seed=seed).eval()
    assert all(float(p.detach().abs().max()) > 0 for n, p in m.named_parameters() if ".conv4.3." in n)
    return m


@torch.no_grad()
def seeded_unet_on_device(cfg, seed, device, cls=I2VGenUNetRef):
    """seeded_unet for models too large to draw on the CPU in a test's time: synthetic.seeded_init's distributions from ONE generator on
    the device -- >= 2-D weights N(0, 1 / fan_in), biases N(0, 0.1^2), norm scales 1 + N(0, 0.1^2), rounded to fp16-representable values"""
    with torch.device(device):
        m = cls(**cfg)
    g = torch.Generator(device=device).manual_seed(seed)
    for name, p in m.named_parameters():
        if p.dim() >= 2:
            v = torch.randn(p.shape, generator=g, device=p.device) / p[0].numel() ** 0.5
        elif name.rsplit(".", 1)[-1] == "weight":
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        else:
            v = 0.1 * torch.randn(p.shape, generator=g, device=p.device)
        p.copy_(v.half().float())
    return m.to(device).eval()


def skip_shapes(cfg, B, F, h, w):
    """[(channels, h, w)] of the skips in the reference's order, and the mid block's"""
    boc, lpb = tuple(cfg["block_out_channels"]), cfg["layers_per_block"]
    out = [(boc[0], h, w)]
    for i, c in enumerate(boc):
        out += [(c, h >> i, w >> i)] * lpb
        if i + 1 < len(boc):
            out.append((c, h >> (i + 1), w >> (i + 1)))
    return out, (boc[-1], h >> (len(boc) - 1), w >> (len(boc) - 1))


def seeded_inputs(cfg, B, F, h, w, seed=7, residuals=None, text_len=77, res_dtype=torch.float16):
    """fp16-representable inputs: sample and image_latents [B, 4, F, h, w], timestep and fps [B], image_embeddings [B, cross],
    encoder_hidden_states [B, text_len, cross]; residuals: None, "4d" ((b f) c h w) or "5d" (b c f h w) -> the down residuals and the mid
    one, in res_dtype"""
    from ctrl_adapter_amd.synthetic import seeded_tensor
    cross = cfg["cross_attention_dim"]
    inp = dict(sample=seeded_tensor((B, cfg["in_channels"], F, h, w), seed),
               timestep=torch.tensor([37.0, 501.0, 12.0, 999.0][:B] if B <= 4 else [float(10 + 7 * i) for i in range(B)]),
               fps=torch.tensor([16.0, 8.0, 24.0, 30.0][:B] if B <= 4 else [float(8 + i) for i in range(B)]),
               image_latents=seeded_tensor((B, 4, F, h, w), seed + 2),
               image_embeddings=seeded_tensor((B, cross), seed + 3),
               encoder_hidden_states=seeded_tensor((B, text_len, cross), seed + 1))
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
