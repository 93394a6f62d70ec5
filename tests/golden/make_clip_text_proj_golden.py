"""Records tests/golden/clip_text_proj.pt from transformers' own CLIPTextModelWithProjection (modeling_clip, eager attention, fp32,
CPU) with the seeded synthetic weights (ctrl_adapter_amd.synthetic.seeded_init, keyed by the names of tests/clip_text_proj_ref.py):

  tiny   2 layers, hidden 128, 2 heads, projection 96, exact gelu, vocab 1000 at B = 2: text_embeds, last hidden state and
         hidden_states[-2] stored whole
  bigg   OpenCLIP ViT-bigG's widths (hidden 1280, 20 heads, intermediate 5120, projection 1280, vocab 49408) at 2 layers, B = 2:
         check_digest digests
  each for both pooled-row rules: eos_token_id = 2 (argmax of the ids) and a real eos id (first position)

Run in an environment with transformers:
    python tests/golden/make_clip_text_proj_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from clip_text_proj_ref import BIGG, TINY_PROJ, CLIPTextProjRef  # noqa: E402
from clip_text_ref import seeded_ids  # noqa: E402
from make_clip_text_golden import digest  # noqa: E402

WEIGHT_SEED = 43
EOS_REAL = 500
BIGG_GOLDEN = dict(BIGG, num_hidden_layers=2)


def hf_model(cfg, sd):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    c = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                       projection_dim=cfg["projection_dim"], num_hidden_layers=cfg["num_hidden_layers"],
                       num_attention_heads=cfg["num_attention_heads"], max_position_embeddings=cfg["max_position_embeddings"],
                       layer_norm_eps=cfg["layer_norm_eps"], eos_token_id=cfg["eos_token_id"], bos_token_id=0, pad_token_id=1,
                       hidden_act=cfg["hidden_act"])
    c._attn_implementation = "eager"
    m = CLIPTextModelWithProjection(c).eval()
    m.load_state_dict(sd, strict=True)
    return m


def seeded_state(cfg):
    import ctrl_adapter_amd.synthetic as syn
    ref = syn.seeded_init(CLIPTextProjRef(**cfg), seed=WEIGHT_SEED)
    return {k: v.clone() for k, v in ref.state_dict().items()}


@torch.no_grad()
def record(cfg, N, full):
    sd = seeded_state(cfg)
    out = {}
    for rule in ("argmax", "eos"):
        c = dict(cfg, eos_token_id=2 if rule == "argmax" else EOS_REAL)
        ids = seeded_ids(N, 77, cfg["vocab_size"], seed=7, eos=None if rule == "argmax" else EOS_REAL)
        r = hf_model(c, sd)(ids, output_hidden_states=True)
        out[rule] = dict(ids=ids, eos_token_id=c["eos_token_id"], text_embeds=digest(r.text_embeds, full=full),
                         last=digest(r.last_hidden_state, full=full and rule == "argmax"), penultimate=digest(r.hidden_states[-2]))
    return out


def main():
    import transformers
    g = dict(transformers_version=transformers.__version__, weight_seed=WEIGHT_SEED, tiny_cfg=TINY_PROJ, bigg_cfg=BIGG_GOLDEN,
             tiny=record(TINY_PROJ, 2, True), bigg=record(BIGG_GOLDEN, 2, False))
    path = os.path.join(HERE, "clip_text_proj.pt")
    torch.save(g, path)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
