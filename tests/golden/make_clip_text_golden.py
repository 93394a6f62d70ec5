"""Records tests/golden/clip_text.pt from transformers' own CLIPTextModel (modeling_clip, eager attention, fp32, CPU) with the seeded
synthetic weights (ctrl_adapter_amd.synthetic.seeded_init, keyed by the transformers 4.x names of tests/clip_text_ref.py):

  tiny   2 layers, hidden 128, 2 heads, vocab 1000 at B = 2: last hidden state (argmax rule) and pooled outputs stored whole
  sd15   SD-1.5's text tower (12 layers, hidden 768, vocab 49408) at B = 4: check_digest digests
  each for both pooled-row rules: eos_token_id = 2 (argmax of the ids, SD-1.5's legacy config) and a real eos id (first position)

Run in an environment with transformers (>= 4.x; the 5.x layout without the `text_model.` prefix is handled):
    python tests/golden/make_clip_text_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from clip_text_ref import CLIPTextRef, SD15, TINY, seeded_ids  # noqa: E402

WEIGHT_SEED = 41
EOS_REAL = {"tiny": 500, "sd15": 500}     # a real eos id (first-position rule) distinct from the argmax position


def digest(t, full=False):
    """the digest format of make_golden.py / helpers.check_digest: strided samples + sums (+ the whole tensor when full)"""
    t = t.detach().float().contiguous()
    flat = t.reshape(-1)
    step = max(1, flat.numel() // 4096)
    d = dict(shape=list(t.shape), sum=float(flat.double().sum()), abssum=float(flat.double().abs().sum()),
             step=step, samples=flat[::step][:4096].clone())
    if full:
        d["full"] = t.clone()
    return d


def hf_model(cfg, sd):
    from transformers import CLIPTextConfig, CLIPTextModel
    c = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                       num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                       max_position_embeddings=cfg["max_position_embeddings"], layer_norm_eps=cfg["layer_norm_eps"],
                       eos_token_id=cfg["eos_token_id"], bos_token_id=0, pad_token_id=1, hidden_act="quick_gelu")
    c._attn_implementation = "eager"
    m = CLIPTextModel(c).eval()
    keys = set(m.state_dict())
    prefixed = any(k.startswith("text_model.") for k in keys)
    m.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in sd.items()}, strict=True)
    return m


def seeded_state(cfg):
    import ctrl_adapter_amd.synthetic as syn
    ref = syn.seeded_init(CLIPTextRef(**cfg), seed=WEIGHT_SEED)
    return {k: v.clone() for k, v in ref.state_dict().items()}


@torch.no_grad()
def record(name, cfg, N, full):
    sd = seeded_state(cfg)
    out = {}
    for rule in ("argmax", "eos"):
        c = dict(cfg, eos_token_id=2 if rule == "argmax" else EOS_REAL[name])
        ids = seeded_ids(N, 77, cfg["vocab_size"], seed=7, eos=None if rule == "argmax" else c["eos_token_id"])
        m = hf_model(c, sd)
        r = m(ids, output_hidden_states=True)
        fl = getattr(m, "text_model", m).final_layer_norm
        skip1 = fl(r.hidden_states[-2])
        # (whole tensors where `full`: the last hidden state of the argmax rule and every pooled output -- the file stays < 300 KB)
        out[rule] = dict(ids=ids, eos_token_id=c["eos_token_id"], last=digest(r.last_hidden_state, full=full and rule == "argmax"),
                         pooled=digest(r.pooler_output, full=full), clip_skip1=digest(skip1))
    return out


def main():
    import transformers
    g = dict(transformers_version=transformers.__version__, weight_seed=WEIGHT_SEED, tiny_cfg=TINY, sd15_cfg=SD15,
             tiny=record("tiny", TINY, 2, True), sd15=record("sd15", SD15, 4, False))
    path = os.path.join(HERE, "clip_text.pt")
    torch.save(g, path)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
