"""fp32 PyTorch restatement of transformers' CLIPTextModel (modeling_clip: CLIPTextTransformer) with the transformers 4.x state-dict
keys (`text_model.` prefix, as SD-1.5's text_encoder stores them): the reference the GPU tests compare the HIP encoder with, so the
GPU box needs no transformers.  Pinned against transformers itself by tests/golden/clip_text.pt and, where transformers is installed,
live (tests/test_text_encoder_host.py).  Same module interface as ctrl_adapter_amd.CLIPTextModel, so encode_controlnet_prompt runs
over either."""
import math

import torch
from torch import nn


class _Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


class _Attn(nn.Module):
    def __init__(self, C, heads):
        super().__init__()
        self.heads = heads
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(C, C) for _ in range(4))

    def forward(self, x):
        N, L, C = x.shape
        D = C // self.heads

        def split(t):
            return t.view(N, L, self.heads, D).transpose(1, 2)

        q, k, v = split(self.q_proj(x)), split(self.k_proj(x)), split(self.v_proj(x))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(D)
        mask = torch.ones(L, L, dtype=torch.bool, device=x.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
        o = s.softmax(-1) @ v
        return self.out_proj(o.transpose(1, 2).reshape(N, L, C))


class _Mlp(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)

    def forward(self, x):
        h = self.fc1(x)
        return self.fc2(h * torch.sigmoid(1.702 * h))


class _Layer(nn.Module):
    def __init__(self, C, I, heads, eps):
        super().__init__()
        self.self_attn = _Attn(C, heads)
        self.layer_norm1 = nn.LayerNorm(C, eps=eps)
        self.mlp = _Mlp(C, I)
        self.layer_norm2 = nn.LayerNorm(C, eps=eps)

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm1(x))
        return x + self.mlp(self.layer_norm2(x))


class _Embeddings(nn.Module):
    def __init__(self, V, C, P):
        super().__init__()
        self.token_embedding = nn.Embedding(V, C)
        self.position_embedding = nn.Embedding(P, C)


class _Encoder(nn.Module):
    def __init__(self, C, I, heads, layers, eps):
        super().__init__()
        self.layers = nn.ModuleList(_Layer(C, I, heads, eps) for _ in range(layers))


class _TextTransformer(nn.Module):
    def __init__(self, V, C, I, heads, layers, P, eps):
        super().__init__()
        self.embeddings = _Embeddings(V, C, P)
        self.encoder = _Encoder(C, I, heads, layers, eps)
        self.final_layer_norm = nn.LayerNorm(C, eps=eps)


class CLIPTextRef(nn.Module):
    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                 max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=49407, **unused):
        super().__init__()
        self.config = _Cfg(vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                           num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                           max_position_embeddings=max_position_embeddings, layer_norm_eps=layer_norm_eps, eos_token_id=eos_token_id,
                           hidden_act="quick_gelu")
        self.text_model = _TextTransformer(vocab_size, hidden_size, intermediate_size, num_attention_heads, num_hidden_layers,
                                           max_position_embeddings, layer_norm_eps)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True):
        assert attention_mask is None
        tm = self.text_model
        ids = input_ids.to(tm.embeddings.token_embedding.weight.device).long()
        L = ids.shape[1]
        x = tm.embeddings.token_embedding(ids) + tm.embeddings.position_embedding.weight[:L]
        hs = [x]
        for layer in tm.encoder.layers:
            x = layer(x)
            hs.append(x)
        last = tm.final_layer_norm(x)
        if self.config.eos_token_id == 2:
            idx = ids.argmax(-1)
        else:
            idx = (ids == self.config.eos_token_id).int().argmax(-1)
        pooled = last[torch.arange(last.shape[0], device=last.device), idx]
        return (last, pooled) + ((tuple(hs),) if output_hidden_states else ())


SD15 = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
            max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)
TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)


def seeded_ids(N, L, vocab, seed, eos=None, pad_from=None):
    """token ids shaped like a tokenizer's: bos 49406-like start, random body, an end token, padding after it.  eos=None: the legacy
    rule's layout (the end token is the LARGEST id, vocab - 1); else the end token is `eos` and the body avoids it"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 2, (N, L), generator=g)
    end = vocab - 1 if eos is None else eos
    if eos is not None:
        ids[ids == eos] = 3
    for n in range(N):
        stop = int(torch.randint(2, L, (1,), generator=g)) if pad_from is None else pad_from
        ids[n, 0] = vocab - 2
        ids[n, stop] = end
        ids[n, stop + 1:] = end if eos is None else 0
    return ids
