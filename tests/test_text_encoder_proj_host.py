"""SDXL prompt encoding, host side (no GPU): the projection restatement against transformers (recorded golden and live), the ext C ABI,
CLIPTextModelWithProjection's configuration / state-dict / persistence handling, and encode_sdxl_prompt against a verbatim transcription
of the SDXL pipeline's encode_prompt over restatement encoders."""
import ctypes
import json
import os
import subprocess
import tempfile

import pytest
import torch

from helpers import ROOT, check_digest, load_golden
from clip_text_proj_ref import BIGG, TINY_PROJ, CLIPTextProjRef
from clip_text_ref import TINY, CLIPTextRef
from test_text_encoder_host import StubTokenizer

EXT_SYMBOLS = ["ctrl_text_encoder_create_ext", "ctrl_text_encoder_forward_ext", "ctrl_text_gemm_ws_bytes", "ctrl_op_text_gemm"]


def seeded(cls, cfg, seed):
    from ctrl_adapter_amd.synthetic import seeded_init
    return seeded_init(cls(**cfg).eval(), seed=seed)


def test_ext_symbols_exported():
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ctrl_hip.h")).read()
    for name in EXT_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert name + "(" in header, name
        assert hasattr(lib, name), "libctrlhip.so does not export %s" % name


def test_ext_struct_size_and_abi_unchanged():
    from ctrl_adapter_amd import _lib
    src = ('#include "ctrl_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %d\\n", sizeof(ctrl_text_encoder_ext), '
           'sizeof(ctrl_text_encoder_config), CTRL_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        ext, cfg, ver = (int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split())
    assert ext == ctypes.sizeof(_lib.TextEncoderExt) == 16
    assert cfg == 32 and ver == 11 == _lib.ABI_VERSION


@pytest.mark.parametrize("which", ["tiny", "bigg"])
@pytest.mark.parametrize("rule", ["argmax", "eos"])
@torch.no_grad()
def test_restatement_matches_transformers_golden(which, rule):
    g = load_golden("clip_text_proj.pt")
    rec = g[which][rule]
    cfg = dict(g["%s_cfg" % which], eos_token_id=rec["eos_token_id"])
    ref = seeded(CLIPTextProjRef, cfg, g["weight_seed"])
    out = ref(rec["ids"], output_hidden_states=True)
    check_digest(out[0], rec["text_embeds"], 1e-5, "%s/%s text_embeds" % (which, rule))
    check_digest(out[1], rec["last"], 1e-5, "%s/%s last" % (which, rule))
    check_digest(out.hidden_states[-2], rec["penultimate"], 1e-5, "%s/%s hidden_states[-2]" % (which, rule))


def test_golden_rules_pick_different_rows():
    g = load_golden("clip_text_proj.pt")
    for which in ("tiny", "bigg"):
        rec = g[which]["eos"]
        ids = rec["ids"]
        assert not torch.equal((ids == rec["eos_token_id"]).int().argmax(-1), ids.argmax(-1))


@torch.no_grad()
def test_restatement_matches_live_transformers():
    tr = pytest.importorskip("transformers")
    for hidden_act in ("gelu", "quick_gelu"):
        cfg = dict(TINY_PROJ, hidden_act=hidden_act, eos_token_id=500)
        ref = seeded(CLIPTextProjRef, cfg, 3)
        c = tr.CLIPTextConfig(**{k: v for k, v in cfg.items()}, bos_token_id=0, pad_token_id=1)
        c._attn_implementation = "eager"
        hf = tr.CLIPTextModelWithProjection(c).eval()
        hf.load_state_dict(ref.state_dict())
        from clip_text_ref import seeded_ids
        ids = seeded_ids(3, 77, cfg["vocab_size"], seed=5, eos=500)
        a, b = ref(ids, output_hidden_states=True), hf(ids, output_hidden_states=True)
        for x, y in ((a[0], b.text_embeds), (a[1], b.last_hidden_state), (a.hidden_states[-2], b.hidden_states[-2])):
            assert ((x - y).abs().max() / y.abs().max()).item() <= 1e-5


@pytest.mark.parametrize("kw", [dict(hidden_act="relu"), dict(hidden_size=768, num_attention_heads=8), dict(max_position_embeddings=78),
                                dict(hidden_size=2112, num_attention_heads=33), dict(intermediate_size=520)])
def test_unsupported_configs_refused(kw):
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError, match="unsupported"):
        P.CLIPTextModelWithProjection(**dict(TINY_PROJ, **kw))


def test_bigg_and_quick_gelu_configs_accepted():
    import ctrl_adapter_amd as P
    m = P.CLIPTextModelWithProjection(**dict(BIGG, num_hidden_layers=1))
    assert m.config.projection_dim == 1280 and m.config.hidden_act == "gelu" and m.gemm_form in (0, 1)
    assert m.state_dict()["text_projection.weight"].shape == (1280, 1280)
    q = P.CLIPTextModelWithProjection(**dict(TINY_PROJ, hidden_act="quick_gelu"), gemm_form=0)
    assert q.gemm_form == 0 and q._ext.hidden_act == 0 and q._ext.projection_dim == 96
    # CLIPTextModel keeps its limits
    with pytest.raises(ValueError, match="unsupported"):
        P.CLIPTextModel(**dict(TINY, hidden_act="gelu"))


def test_both_state_dict_layouts():
    import ctrl_adapter_amd as P
    ref = seeded(CLIPTextProjRef, TINY_PROJ, 5)
    sd = ref.state_dict()
    m = P.CLIPTextModelWithProjection(**TINY_PROJ)
    assert set(m.state_dict()) == set(sd) and m.dtype == torch.float32
    m.load_state_dict(dict(sd, **{"text_model.embeddings.position_ids": torch.arange(77)[None]}))
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    m5 = P.CLIPTextModelWithProjection(**TINY_PROJ)
    m5.load_state_dict({(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()})
    for k, v in sd.items():
        assert torch.equal(m5.state_dict()[k], v), k
    with pytest.raises(RuntimeError):
        m5.load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"})
    with pytest.raises(ValueError, match="attention_mask"):
        m(torch.zeros(1, 77, dtype=torch.long), attention_mask=torch.ones(1, 77))


@pytest.mark.parametrize("variant", [None, "fp16"])
def test_save_and_from_pretrained(tmp_path, variant):
    import ctrl_adapter_amd as P
    ref = seeded(CLIPTextProjRef, TINY_PROJ, 6)
    m = P.CLIPTextModelWithProjection(**TINY_PROJ)
    m.load_state_dict(ref.state_dict())
    if variant:
        m = m.half()
    m.save_pretrained(str(tmp_path / "text_encoder_2"), variant=variant)
    files = sorted(os.listdir(tmp_path / "text_encoder_2"))
    assert files == ["config.json", "model%s.safetensors" % (".%s" % variant if variant else "")]
    cfg = json.load(open(tmp_path / "text_encoder_2" / "config.json"))
    assert cfg["architectures"] == ["CLIPTextModelWithProjection"] and cfg["projection_dim"] == 96 and cfg["hidden_act"] == "gelu"
    m2 = P.CLIPTextModelWithProjection.from_pretrained(str(tmp_path), subfolder="text_encoder_2", torch_dtype=torch.float16,
                                                       variant=variant)
    assert m2.dtype == torch.float16 and m2.config.projection_dim == 96
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k].float(), v), k


# ------------------------------------------------------------------------------------------ encode_sdxl_prompt
class HFLikeCLIP(CLIPTextRef):
    """the CLIP-L restatement with transformers' output object (the method reads `.hidden_states`)"""

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True):
        from clip_text_proj_ref import _Out
        last, pooled, hs = super().forward(input_ids, output_hidden_states=True)
        o = _Out(last, pooled, hs if output_hidden_states else None)
        return o


class Pipe:
    """what the transcription reads from `self`"""

    def __init__(self, tokenizers, encoders, force_zeros=True):
        self.tokenizer, self.tokenizer_2 = (tokenizers[0], tokenizers[1]) if len(tokenizers) == 2 else (None, tokenizers[0])
        self.text_encoder, self.text_encoder_2 = (encoders[0], encoders[1]) if len(encoders) == 2 else (None, encoders[0])

        class Cfg:
            force_zeros_for_empty_prompt = force_zeros
        self.config = Cfg()


def pipeline_encode_prompt(self, prompt, prompt_2=None, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True,
                           negative_prompt=None, negative_prompt_2=None, prompt_embeds=None, negative_prompt_embeds=None,
                           pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, lora_scale=None, clip_skip=None):
    """the SDXL pipeline's encode_prompt (sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:282-515), transcribed verbatim but for
    the LoRA scaling, textual inversion and the truncation warning (no effect on the values)"""
    prompt = [prompt] if isinstance(prompt, str) else prompt
    if prompt is not None:
        batch_size = len(prompt)
    else:
        batch_size = prompt_embeds.shape[0]
    tokenizers = [self.tokenizer, self.tokenizer_2] if self.tokenizer is not None else [self.tokenizer_2]
    text_encoders = [self.text_encoder, self.text_encoder_2] if self.text_encoder is not None else [self.text_encoder_2]
    if prompt_embeds is None:
        prompt_2 = prompt_2 or prompt
        prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
        prompt_embeds_list = []
        prompts = [prompt, prompt_2]
        for prompt, tokenizer, text_encoder in zip(prompts, tokenizers, text_encoders):
            text_inputs = tokenizer(prompt, padding="max_length", max_length=tokenizer.model_max_length, truncation=True,
                                    return_tensors="pt")
            text_input_ids = text_inputs.input_ids
            prompt_embeds = text_encoder(text_input_ids.to(device), output_hidden_states=True)
            pooled_prompt_embeds = prompt_embeds[0]
            if clip_skip is None:
                prompt_embeds = prompt_embeds.hidden_states[-2]
            else:
                prompt_embeds = prompt_embeds.hidden_states[-(clip_skip + 2)]
            prompt_embeds_list.append(prompt_embeds)
        prompt_embeds = torch.concat(prompt_embeds_list, dim=-1)
    zero_out_negative_prompt = negative_prompt is None and self.config.force_zeros_for_empty_prompt
    if do_classifier_free_guidance and negative_prompt_embeds is None and zero_out_negative_prompt:
        negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
    elif do_classifier_free_guidance and negative_prompt_embeds is None:
        negative_prompt = negative_prompt or ""
        negative_prompt_2 = negative_prompt_2 or negative_prompt
        negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
        if prompt is not None and type(prompt) is not type(negative_prompt):
            raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != {type(prompt)}.")
        elif batch_size != len(negative_prompt):
            raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has "
                             f"batch size {batch_size}. Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
        else:
            uncond_tokens = [negative_prompt, negative_prompt_2]
        negative_prompt_embeds_list = []
        for negative_prompt, tokenizer, text_encoder in zip(uncond_tokens, tokenizers, text_encoders):
            max_length = prompt_embeds.shape[1]
            uncond_input = tokenizer(negative_prompt, padding="max_length", max_length=max_length, truncation=True, return_tensors="pt")
            negative_prompt_embeds = text_encoder(uncond_input.input_ids.to(device), output_hidden_states=True)
            negative_pooled_prompt_embeds = negative_prompt_embeds[0]
            negative_prompt_embeds = negative_prompt_embeds.hidden_states[-2]
            negative_prompt_embeds_list.append(negative_prompt_embeds)
        negative_prompt_embeds = torch.concat(negative_prompt_embeds_list, dim=-1)
    if self.text_encoder_2 is not None:
        prompt_embeds = prompt_embeds.to(dtype=self.text_encoder_2.dtype, device=device)
    bs_embed, seq_len, _ = prompt_embeds.shape
    prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
    prompt_embeds = prompt_embeds.view(bs_embed * num_images_per_prompt, seq_len, -1)
    if do_classifier_free_guidance:
        seq_len = negative_prompt_embeds.shape[1]
        if self.text_encoder_2 is not None:
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=self.text_encoder_2.dtype, device=device)
        negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1)
        negative_prompt_embeds = negative_prompt_embeds.view(batch_size * num_images_per_prompt, seq_len, -1)
    pooled_prompt_embeds = pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)
    if do_classifier_free_guidance:
        negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(
            bs_embed * num_images_per_prompt, -1)
    return prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds


TINY_L = dict(TINY, vocab_size=1000)
TINY_G = dict(TINY_PROJ, hidden_size=192, num_attention_heads=3, projection_dim=64)


@pytest.fixture(scope="module")
def towers():
    torch.set_grad_enabled(False)
    return [seeded(HFLikeCLIP, TINY_L, 11), seeded(CLIPTextProjRef, TINY_G, 12)], [StubTokenizer(1000), StubTokenizer(1000)]


def _same(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        if y is None:
            assert x is None
        else:
            assert x.shape == y.shape and x.dtype == y.dtype
            assert (x - y).abs().max().item() <= 1e-5 * max(y.abs().max().item(), 1.0), (x - y).abs().max()


CASES = [
    dict(prompt="a cat"),
    dict(prompt=["a cat", "two dogs"], negative_prompt="blurry"),
    dict(prompt=["a cat", "two dogs"], negative_prompt=["blurry", "dark"], negative_prompt_2=["x", "yy"]),
    dict(prompt="a cat", prompt_2="a cat in bigG", negative_prompt="bad", clip_skip=1),
    dict(prompt=["a", "bb"], clip_skip=1, num_images_per_prompt=2),
    dict(prompt="a cat", negative_prompt="bad", num_images_per_prompt=2),
    dict(prompt="a cat", do_classifier_free_guidance=False),
    dict(prompt=["a", "bb"], do_classifier_free_guidance=False, clip_skip=1, num_images_per_prompt=2),
]


@pytest.mark.parametrize("force_zeros", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_encode_sdxl_prompt_matches_pipeline(towers, case, force_zeros):
    import ctrl_adapter_amd as P
    encs, toks = towers
    kw = CASES[case]
    want = pipeline_encode_prompt(Pipe(toks, encs, force_zeros), **kw)
    got = P.encode_sdxl_prompt(toks, encs, force_zeros_for_empty_prompt=force_zeros, **kw)
    _same(got, want)


def test_encode_sdxl_prompt_single_encoder_and_given_embeds(towers):
    import ctrl_adapter_amd as P
    encs, toks = towers
    _same(P.encode_sdxl_prompt(toks[1:], encs[1:], "a cat", negative_prompt="no", force_zeros_for_empty_prompt=False),
          pipeline_encode_prompt(Pipe(toks[1:], encs[1:], False), "a cat", negative_prompt="no"))
    pe, _, pp, _ = pipeline_encode_prompt(Pipe(toks, encs), ["a", "b"], do_classifier_free_guidance=False)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pp, negative_prompt=["x", "y"])
    _same(P.encode_sdxl_prompt(toks, encs, None, force_zeros_for_empty_prompt=False, **kw),
          pipeline_encode_prompt(Pipe(toks, encs, False), None, **kw))


def test_encode_sdxl_prompt_errors(towers):
    import ctrl_adapter_amd as P
    encs, toks = towers
    for kw, exc in ((dict(prompt=["a", "b"], negative_prompt=("x", "y")), TypeError),
                    (dict(prompt=["a", "b"], negative_prompt=["x"]), ValueError)):
        with pytest.raises(exc):
            pipeline_encode_prompt(Pipe(toks, encs), **kw)
        with pytest.raises(exc):
            P.encode_sdxl_prompt(toks, encs, **kw)
    with pytest.raises(ValueError, match="vocabulary"):
        P.encode_sdxl_prompt([StubTokenizer(5000), toks[1]], encs, "a cat")
