"""CLIP text encoder, host side (no GPU): the C ABI of the new plan, the fp32 restatement against transformers (recorded golden and
live), the mirror's configuration / state-dict handling, and encode_controlnet_prompt's argument handling over the restatement."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from helpers import ROOT, check_digest, load_golden
from clip_text_ref import CLIPTextRef, SD15, TINY, seeded_ids

TEXT_SYMBOLS = ["ctrl_text_encoder_create", "ctrl_text_encoder_destroy", "ctrl_text_encoder_forward", "ctrl_text_encoder_id_status",
                "ctrl_op_text_embed", "ctrl_op_text_attn", "ctrl_op_text_final_ln"]


def seeded_ref(cfg, seed=41, **kw):
    from ctrl_adapter_amd.synthetic import seeded_init
    return seeded_init(CLIPTextRef(**cfg).eval(), seed=seed, **kw)


def test_text_encoder_symbols_exported():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    for name in TEXT_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), "libctrlhip.so does not export %s" % name


def test_text_encoder_config_struct_size():
    from ctrl_adapter_amd import _lib
    src = '#include "ctrl_hip.h"\n#include <stdio.h>\nint main(){printf("%zu\\n", sizeof(ctrl_text_encoder_config));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = int(subprocess.check_output([os.path.join(d, "s")]).decode())
    assert out == ctypes.sizeof(_lib.TextEncoderConfig) == 32


def _golden():
    return load_golden("clip_text.pt")


@pytest.mark.parametrize("which", ["tiny", "sd15"])
@pytest.mark.parametrize("rule", ["argmax", "eos"])
@torch.no_grad()
def test_restatement_matches_transformers_golden(which, rule):
    g = _golden()
    rec = g[which][rule]
    cfg = dict(g["%s_cfg" % which], eos_token_id=rec["eos_token_id"])
    ref = seeded_ref(cfg, seed=g["weight_seed"])
    last, pooled, hs = ref(rec["ids"], output_hidden_states=True)
    check_digest(last, rec["last"], 1e-5, "%s/%s last" % (which, rule))
    check_digest(pooled, rec["pooled"], 1e-5, "%s/%s pooled" % (which, rule))
    check_digest(ref.text_model.final_layer_norm(hs[-2]), rec["clip_skip1"], 1e-5, "%s/%s clip_skip=1" % (which, rule))


def test_golden_rules_pick_different_rows():
    """the two pooled-row rules are told apart by the recorded ids (else the eos case would prove nothing)"""
    g = _golden()
    for which in ("tiny", "sd15"):
        rec = g[which]["eos"]
        ids = rec["ids"]
        first_eos = (ids == rec["eos_token_id"]).int().argmax(-1)
        assert not torch.equal(first_eos, ids.argmax(-1))


@torch.no_grad()
def test_restatement_matches_live_transformers():
    transformers = pytest.importorskip("transformers")
    from transformers import CLIPTextConfig, CLIPTextModel
    for eos in (2, 500):
        cfg = dict(TINY, eos_token_id=eos)
        ref = seeded_ref(cfg, seed=3)
        c = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                           num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                           max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=eos, bos_token_id=0, pad_token_id=1)
        hf = CLIPTextModel(c).eval()
        prefixed = any(k.startswith("text_model.") for k in hf.state_dict())
        hf.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in ref.state_dict().items()})
        ids = seeded_ids(3, 77, cfg["vocab_size"], seed=11, eos=None if eos == 2 else eos)
        r = hf(ids, output_hidden_states=True)
        last, pooled, hs = ref(ids, output_hidden_states=True)
        for a, b in ((last, r.last_hidden_state), (pooled, r.pooler_output), (hs[-2], r.hidden_states[-2]), (hs[0], r.hidden_states[0])):
            assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-5
        assert transformers.__version__


@pytest.mark.parametrize("kw", [dict(hidden_act="gelu"), dict(hidden_size=768, num_attention_heads=8), dict(max_position_embeddings=78),
                                dict(hidden_size=512, num_attention_heads=4)])
def test_unsupported_configs_refused(kw):
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError, match="unsupported"):
        P.CLIPTextModel(**dict(TINY, **kw))


def test_mirror_interface_and_both_state_dict_layouts():
    import ctrl_adapter_amd as P
    ref = seeded_ref(TINY, seed=5)
    sd4 = ref.state_dict()
    m = P.CLIPTextModel(**TINY)
    assert set(m.state_dict()) == set(sd4)
    assert m.dtype == torch.float32
    assert not hasattr(m.config, "use_attention_mask")
    assert m.config.eos_token_id == 2 and m.config.hidden_size == 128
    # transformers 4.x keys (+ the position_ids buffer SD-1.5's checkpoint carries)
    m.load_state_dict(dict(sd4, **{"text_model.embeddings.position_ids": torch.arange(77)[None]}))
    for k, v in sd4.items():
        assert torch.equal(m.state_dict()[k], v), k
    # transformers 5.x keys: no `text_model.` prefix
    m5 = P.CLIPTextModel(**TINY)
    m5.load_state_dict({k[len("text_model."):]: v for k, v in sd4.items()})
    for k, v in sd4.items():
        assert torch.equal(m5.state_dict()[k], v), k
    with pytest.raises(RuntimeError):
        m5.load_state_dict({k: v for k, v in sd4.items() if "fc2" not in k})
    assert isinstance(m.text_model.final_layer_norm, torch.nn.Module)
    with pytest.raises(ValueError, match="attention_mask"):
        m(torch.zeros(1, 77, dtype=torch.long), attention_mask=torch.ones(1, 77))


def test_mirror_save_and_from_pretrained(tmp_path):
    import ctrl_adapter_amd as P
    ref = seeded_ref(TINY, seed=6)
    m = P.CLIPTextModel(**TINY)
    m.load_state_dict(ref.state_dict())
    m.save_pretrained(str(tmp_path / "text_encoder"))
    m2 = P.CLIPTextModel.from_pretrained(str(tmp_path), subfolder="text_encoder", torch_dtype=torch.float16)
    assert m2.dtype == torch.float16 and m2.config.vocab_size == TINY["vocab_size"]
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k].float(), v), k        # seeded weights are fp16-representable


# ------------------------------------------------------------------------------------------ encode_controlnet_prompt
class StubTokenizer:
    """CLIPTokenizer-shaped: bos, one id per character, eos, padded with eos to max_length (truncation keeps the eos)"""
    model_max_length = 77

    def __init__(self, vocab):
        self.vocab = vocab

    def encode(self, text, max_length):
        body = [3 + (ord(c) * 7) % (self.vocab - 5) for c in text][: max_length - 2]
        ids = [self.vocab - 2] + body + [self.vocab - 1]
        return ids + [self.vocab - 1] * (max_length - len(ids))

    def __call__(self, texts, padding, max_length, truncation, return_tensors):
        assert padding == "max_length" and truncation and return_tensors == "pt"
        texts = [texts] if isinstance(texts, str) else texts

        class R:
            pass
        r = R()
        r.input_ids = torch.tensor([self.encode(t, max_length) for t in texts], dtype=torch.long)
        return r


@pytest.fixture(scope="module")
def tiny_ref():
    return seeded_ref(TINY, seed=9)


def _direct(ref, tok, texts, clip_skip=None):
    ids = tok(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    last, pooled, hs = ref(ids, output_hidden_states=True)
    if clip_skip is not None:
        last = ref.text_model.final_layer_norm(hs[-(clip_skip + 1)])
    return last, pooled


@torch.no_grad()
def test_encode_prompt_argument_errors(tiny_ref):
    from ctrl_adapter_amd import encode_controlnet_prompt
    tok = StubTokenizer(TINY["vocab_size"])
    with pytest.raises(TypeError):
        encode_controlnet_prompt(tok, tiny_ref, ["a cat"], "cpu", 1, True, negative_prompt="blurry")
    with pytest.raises(ValueError):
        encode_controlnet_prompt(tok, tiny_ref, ["a cat", "a dog"], "cpu", 1, True, negative_prompt=["blurry"])
    bad = StubTokenizer(TINY["vocab_size"] + 10)      # ids beyond the encoder's vocabulary are refused on the host
    with pytest.raises(ValueError, match="vocabulary"):
        encode_controlnet_prompt(bad, tiny_ref, "a cat", "cpu", 1, False)


@pytest.mark.parametrize("clip_skip", [None, 1])
@torch.no_grad()
def test_encode_prompt_repeat_and_cfg_order(tiny_ref, clip_skip):
    from ctrl_adapter_amd import encode_controlnet_prompt
    tok = StubTokenizer(TINY["vocab_size"])
    pe, ne, pp, npool = encode_controlnet_prompt(tok, tiny_ref, ["a cat", "a red dog"], "cpu", 3, True,
                                                 negative_prompt=["blurry", "dark"], clip_skip=clip_skip)
    assert pe.shape == (6, 77, 128) and ne.shape == (6, 77, 128) and pp.shape == (6, 128) and npool.shape == (6, 128)
    want_p, want_pp = _direct(tiny_ref, tok, ["a cat", "a red dog"], clip_skip)
    want_n, want_np = _direct(tiny_ref, tok, ["blurry", "dark"])          # negatives never take clip_skip
    order = [0, 0, 0, 1, 1, 1]
    torch.testing.assert_close(pe, want_p[order], rtol=0, atol=1e-5)
    torch.testing.assert_close(pp, want_pp[order], rtol=0, atol=1e-5)
    torch.testing.assert_close(ne, want_n[order], rtol=0, atol=1e-5)
    torch.testing.assert_close(npool, want_np[order], rtol=0, atol=1e-5)
    # default negative: [""] * batch
    pe2, ne2, _, _ = encode_controlnet_prompt(tok, tiny_ref, "a cat", "cpu", 2, True)
    torch.testing.assert_close(ne2, _direct(tiny_ref, tok, [""])[0][[0, 0]], rtol=0, atol=1e-5)
    assert pe2.dtype == tiny_ref.dtype


@torch.no_grad()
def test_encode_prompt_none_where_the_reference_never_assigns(tiny_ref):
    """deviation: the reference raises UnboundLocalError in these cases; here the unassigned values are None"""
    from ctrl_adapter_amd import encode_controlnet_prompt
    tok = StubTokenizer(TINY["vocab_size"])
    pe, ne, pp, npool = encode_controlnet_prompt(tok, tiny_ref, "a cat", "cpu", 2, False)
    assert ne is None and npool is None and pe.shape == (2, 77, 128) and pp.shape == (2, 128)
    given = _direct(tiny_ref, tok, ["x"])[0]
    pe, ne, pp, npool = encode_controlnet_prompt(tok, tiny_ref, None, "cpu", 2, True, prompt_embeds=given, lora_scale=0.7)
    assert pp is None and torch.equal(pe, given[[0, 0]])
    torch.testing.assert_close(ne, _direct(tiny_ref, tok, [""])[0][[0, 0]], rtol=0, atol=1e-5)
    assert npool.shape == (2, 128)
    pe, ne, pp, npool = encode_controlnet_prompt(tok, tiny_ref, "a cat", "cpu", 1, True, negative_prompt_embeds=given)
    assert npool is None and torch.equal(ne, given)
