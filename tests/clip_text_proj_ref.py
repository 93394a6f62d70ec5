"""fp32 PyTorch restatement of transformers' CLIPTextModelWithProjection (SDXL's text_encoder_2, OpenCLIP ViT-bigG): the text tower of
tests/clip_text_ref.py with `hidden_act` quick_gelu or exact gelu and the bias-free `text_projection` of the pooled row.  Pinned
against transformers by tests/golden/clip_text_proj.pt.  Same module interface as ctrl_adapter_amd.CLIPTextModelWithProjection
([0] text_embeds, [1] last_hidden_state, .hidden_states), so encode_sdxl_prompt runs over either."""
import torch
import torch.nn.functional as F
from torch import nn

from clip_text_ref import CLIPTextRef, _Cfg


class _Out(tuple):
    def __new__(cls, text_embeds, last_hidden_state, hidden_states=None):
        self = super().__new__(cls, (text_embeds, last_hidden_state) + ((hidden_states,) if hidden_states is not None else ()))
        self.text_embeds, self.last_hidden_state, self.hidden_states = text_embeds, last_hidden_state, hidden_states
        return self


class _GeluMlp(nn.Module):
    def __init__(self, fc1, fc2):
        super().__init__()
        self.fc1, self.fc2 = fc1, fc2

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class CLIPTextProjRef(nn.Module):
    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                 num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407,
                 **unused):
        super().__init__()
        tower = CLIPTextRef(vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                            num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                            max_position_embeddings=max_position_embeddings, layer_norm_eps=layer_norm_eps, eos_token_id=eos_token_id)
        self.config = _Cfg(dict(tower.config, hidden_act=hidden_act, projection_dim=projection_dim))
        self.text_model = tower.text_model
        self._tower = [tower]          # (not a submodule: its parameters are self.text_model's)
        if hidden_act == "gelu":
            for layer in self.text_model.encoder.layers:
                layer.mlp = _GeluMlp(layer.mlp.fc1, layer.mlp.fc2)
        self.text_projection = nn.Linear(hidden_size, projection_dim, bias=False)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True):
        last, pooled, hs = self._tower[0](input_ids, attention_mask=attention_mask, output_hidden_states=True)
        emb = self.text_projection(pooled)
        return _Out(emb, last, hs if output_hidden_states else None)


# OpenCLIP ViT-bigG/14 text tower as SDXL's text_encoder_2/config.json states it
BIGG = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, projection_dim=1280, num_hidden_layers=32, num_attention_heads=20,
            max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2)
TINY_PROJ = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, projection_dim=96, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2)
