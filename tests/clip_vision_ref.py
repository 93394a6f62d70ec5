"""fp32 PyTorch restatement of transformers' CLIPVisionModelWithProjection (the image_encoder of SVD and I2VGen-XL, CLIP ViT-H/14) and of
SVD's image preprocessing (_resize_with_antialiasing: Gaussian blur with reflect padding, then a bicubic align_corners resize).  Our own
code, pinned against transformers and the pipeline's helpers by tests/golden/clip_vision.pt.  Same module interface as
ctrl_adapter_amd.CLIPVisionModelWithProjection ([0] image_embeds, [1] last_hidden_state, .hidden_states)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

# CLIP ViT-H/14, the image_encoder of stabilityai/stable-video-diffusion-img2vid(-xt) and ali-vilab/i2vgen-xl
VIT_H = dict(hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16, image_size=224,
             patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)
TINY = dict(hidden_size=128, intermediate_size=256, projection_dim=96, num_hidden_layers=2, num_attention_heads=2, image_size=56,
            patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)


class _Out(tuple):
    def __new__(cls, image_embeds, last_hidden_state, hidden_states=None):
        self = super().__new__(cls, (image_embeds, last_hidden_state) + ((hidden_states,) if hidden_states is not None else ()))
        self.image_embeds, self.last_hidden_state, self.hidden_states = image_embeds, last_hidden_state, hidden_states
        return self


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _Attn(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(C, C) for _ in range(4))


class _Mlp(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)


class _Layer(nn.Module):
    def __init__(self, C, I, eps):
        super().__init__()
        self.self_attn = _Attn(C)
        self.layer_norm1 = nn.LayerNorm(C, eps=eps)
        self.mlp = _Mlp(C, I)
        self.layer_norm2 = nn.LayerNorm(C, eps=eps)


class CLIPVisionRef(nn.Module):
    def __init__(self, hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12,
                 image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, **unused):
        super().__init__()
        C, I = hidden_size, intermediate_size
        self.config = _Cfg(hidden_size=C, intermediate_size=I, projection_dim=projection_dim, num_hidden_layers=num_hidden_layers,
                           num_attention_heads=num_attention_heads, image_size=image_size, patch_size=patch_size, hidden_act=hidden_act,
                           layer_norm_eps=layer_norm_eps)
        tokens = (image_size // patch_size) ** 2 + 1
        vm = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.zeros(C))
        vm.embeddings.patch_embedding = nn.Conv2d(3, C, patch_size, stride=patch_size, bias=False)
        vm.embeddings.position_embedding = nn.Embedding(tokens, C)
        vm.pre_layrnorm = nn.LayerNorm(C, eps=layer_norm_eps)
        vm.encoder = nn.Module()
        vm.encoder.layers = nn.ModuleList(_Layer(C, I, layer_norm_eps) for _ in range(num_hidden_layers))
        vm.post_layernorm = nn.LayerNorm(C, eps=layer_norm_eps)
        self.vision_model = vm
        self.visual_projection = nn.Linear(C, projection_dim, bias=False)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def _act(self, x):
        if self.config.hidden_act == "gelu":
            return F.gelu(x)
        return x * torch.sigmoid(1.702 * x)

    def forward(self, pixel_values, output_hidden_states=False, return_dict=True):
        vm, cfg = self.vision_model, self.config
        x = pixel_values.to(self.dtype)
        N = x.shape[0]
        patches = vm.embeddings.patch_embedding(x).flatten(2).transpose(1, 2)               # [N, P, C]
        cls = vm.embeddings.class_embedding.view(1, 1, -1).expand(N, 1, -1)
        h = torch.cat([cls, patches], 1) + vm.embeddings.position_embedding.weight[None]
        h = vm.pre_layrnorm(h)
        states = [h]
        heads = cfg.num_attention_heads
        D = cfg.hidden_size // heads
        for layer in vm.encoder.layers:
            a = layer.layer_norm1(h)
            L_ = a.shape[1]
            q = layer.self_attn.q_proj(a).view(N, L_, heads, D).transpose(1, 2)
            k = layer.self_attn.k_proj(a).view(N, L_, heads, D).transpose(1, 2)
            v = layer.self_attn.v_proj(a).view(N, L_, heads, D).transpose(1, 2)
            p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D), -1)
            h = h + layer.self_attn.out_proj((p @ v).transpose(1, 2).reshape(N, L_, -1))
            h = h + layer.mlp.fc2(self._act(layer.mlp.fc1(layer.layer_norm2(h))))
            states.append(h)
        pooled = vm.post_layernorm(h[:, 0])
        emb = self.visual_projection(pooled)
        hs = tuple(states) if output_hidden_states else None
        if not return_dict:
            return (emb, h) + ((hs,) if hs is not None else ())
        return _Out(emb, h, hs)


# ------------------------------------------------------------------------------------------ SVD's preprocessing
def gaussian_taps(n_in, n_out):
    """sigma, kernel size and normalised fp32 taps along one axis, as _resize_with_antialiasing chooses them"""
    sigma = max((n_in / n_out - 1.0) / 2.0, 0.001)
    ks = int(max(2.0 * 2 * sigma, 3))
    if ks % 2 == 0:
        ks += 1
    s = torch.tensor(sigma, dtype=torch.float32)
    x = torch.arange(ks, dtype=torch.float32) - ks // 2
    w = torch.exp(-x.pow(2.0) / (2 * s.pow(2.0)))
    return sigma, ks, w / w.sum()


def resize_with_antialiasing(x, size):
    """x [N, 3, H, W] fp32 -> [N, 3, size]: separable Gaussian blur (reflect padding; x pass, then y pass), then bicubic align_corners"""
    N, Cc, H, W = x.shape
    _, ky, wy = gaussian_taps(H, size[0])
    _, kx, wx = gaussian_taps(W, size[1])
    flat = x.reshape(N * Cc, 1, H, W)
    flat = F.conv2d(F.pad(flat, ((kx - 1) // 2, kx - 1 - (kx - 1) // 2, 0, 0), mode="reflect"), wx.view(1, 1, 1, kx))
    flat = F.conv2d(F.pad(flat, (0, 0, (ky - 1) // 2, ky - 1 - (ky - 1) // 2), mode="reflect"), wy.view(1, 1, ky, 1))
    return F.interpolate(flat.reshape(N, Cc, H, W), size=size, mode="bicubic", align_corners=True)


def svd_preprocess(u8_nhwc, mean, std, size=(224, 224)):
    """the SVD pipeline's _encode_image up to the encoder, for uint8 HWC frames: / 255, * 2 - 1, resize, (x + 1) / 2, CLIP normalise"""
    x = torch.as_tensor(u8_nhwc).float().div(255.0).permute(0, 3, 1, 2)
    x = resize_with_antialiasing(x * 2.0 - 1.0, size)
    x = (x + 1.0) / 2.0
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (x - m) / s


def seeded_pixels(N, S, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (N, S, S, 3), generator=g, dtype=torch.uint8)
    return torch.randn(N, 3, S, S, generator=g)
