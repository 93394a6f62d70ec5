"""CLIPTextModel -- drop-in mirror of the SD-1.5 text encoder (transformers CLIPTextModel, the `text_encoder` that
ControlNetHelper loads at model/ctrl_helper.py:34-41) whose forward runs in libctrlhip (csrc/text.hip, csrc/plan_text.cpp), and
encode_controlnet_prompt -- ControlNetHelper.encode_controlnet_prompt (model/ctrl_helper.py:300-457) with the prompts and the
negative prompts encoded in ONE forward.

State-dict keys are the transformers 4.x layout SD-1.5's text_encoder/model.safetensors stores (`text_model.embeddings....`);
the 5.x layout without the `text_model.` prefix loads as well."""
import torch
from torch import nn

from . import _lib as L
from ._plan import Config, ParamTreeModule


class CLIPTextOutput(tuple):
    """(last_hidden_state, pooler_output[, hidden_states]) with attribute access, indexed like transformers'
    BaseModelOutputWithPooling: [0] last hidden state, [1] pooled, [-1] the tuple of hidden states when they were asked for"""

    def __new__(cls, last_hidden_state, pooler_output, hidden_states=None):
        items = (last_hidden_state, pooler_output) + ((hidden_states,) if hidden_states is not None else ())
        self = super().__new__(cls, items)
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states
        return self


def text_encoder_spec(vocab_size, hidden_size, intermediate_size, num_hidden_layers, max_position_embeddings):
    """(name, shape) of every parameter, transformers 4.x keys"""
    C_, I = hidden_size, intermediate_size
    spec = [("text_model.embeddings.token_embedding.weight", (vocab_size, C_)),
            ("text_model.embeddings.position_embedding.weight", (max_position_embeddings, C_))]
    for i in range(num_hidden_layers):
        p = "text_model.encoder.layers.%d." % i
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            spec += [(p + "self_attn.%s.weight" % proj, (C_, C_)), (p + "self_attn.%s.bias" % proj, (C_,))]
        spec += [(p + "layer_norm1.weight", (C_,)), (p + "layer_norm1.bias", (C_,)),
                 (p + "mlp.fc1.weight", (I, C_)), (p + "mlp.fc1.bias", (I,)),
                 (p + "mlp.fc2.weight", (C_, I)), (p + "mlp.fc2.bias", (C_,)),
                 (p + "layer_norm2.weight", (C_,)), (p + "layer_norm2.bias", (C_,))]
    spec += [("text_model.final_layer_norm.weight", (C_,)), ("text_model.final_layer_norm.bias", (C_,))]
    return spec


def final_layer_norm(x, weight, bias, eps):
    """LayerNorm over the last dim on the device (csrc/text.hip text_final_kernel), output in x's dtype"""
    if not x.is_cuda:
        raise RuntimeError("final_layer_norm: the tensor must live on the GPU; there is no CPU path")
    xc = x.contiguous()
    Cn = xc.shape[-1]
    y = torch.empty_like(xc)
    g = weight.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    b = bias.detach().to(device=xc.device, dtype=torch.float32).contiguous()
    L.check(L.lib().ctrl_op_text_final_ln(L.ptr(xc), L.dtype_code(xc.dtype), xc.numel() // Cn, Cn, L.ptr(g), L.ptr(b), float(eps),
                                          L.ptr(y), L.dtype_code(y.dtype), None, 0, 0, None, L.cur_stream()))
    return y


class _FinalLayerNorm(nn.Module):
    """`text_model.final_layer_norm`: holds the weight / bias and applies them to a tensor (encode_controlnet_prompt's clip_skip
    path calls it on a hidden state, model/ctrl_helper.py:382)"""

    def __init__(self, eps):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        return final_layer_norm(x, self.weight, self.bias, self.eps)


class CLIPTextModel(ParamTreeModule):
    _CREATE, _DESTROY = "ctrl_text_encoder_create", "ctrl_text_encoder_destroy"

    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                 num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                 attention_dropout=0.0, initializer_range=0.02, initializer_factor=1.0, pad_token_id=1, bos_token_id=49406,
                 eos_token_id=49407, **unused):
        super().__init__()
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__", "unused")})
        unsupported = []
        if hidden_act != "quick_gelu":
            unsupported.append("hidden_act %r (quick_gelu only)" % (hidden_act,))
        if num_attention_heads < 1 or hidden_size != 64 * num_attention_heads:
            unsupported.append("head_dim %s (64 only)" % (hidden_size / max(num_attention_heads, 1)))
        if max_position_embeddings > 77:
            unsupported.append("max_position_embeddings %d (<= 77)" % max_position_embeddings)
        if hidden_size > 1024 or intermediate_size % 64:
            unsupported.append("hidden_size > 1024 or intermediate_size not a multiple of 64")
        if unsupported:
            raise ValueError("CLIPTextModel (libctrlhip): unsupported configuration: " + ", ".join(unsupported))
        cfg = L.TextEncoderConfig()
        cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = vocab_size, hidden_size, intermediate_size
        cfg.num_hidden_layers, cfg.num_attention_heads = num_hidden_layers, num_attention_heads
        cfg.max_position_embeddings, cfg.eos_token_id, cfg.layer_norm_eps = max_position_embeddings, eos_token_id, layer_norm_eps
        self._cfg = cfg
        self.add_module("text_model", nn.Module())
        self.text_model.add_module("final_layer_norm", _FinalLayerNorm(layer_norm_eps))
        self._register_spec(text_encoder_spec(vocab_size, hidden_size, intermediate_size, num_hidden_layers, max_position_embeddings),
                            dtype=torch.float32)

    def config_dict(self):
        return dict(self.config, architectures=["CLIPTextModel"], model_type="clip_text_model")

    def load_state_dict(self, state_dict, strict=True, **k):
        """accepts the transformers 4.x keys (`text_model.` prefix, SD-1.5's checkpoints) and the 5.x keys (no prefix); the
        non-persistent `position_ids` buffer some checkpoints carry is dropped"""
        sd = {}
        for key, v in state_dict.items():
            if key.endswith("embeddings.position_ids"):
                continue
            sd[key if key.startswith("text_model.") else "text_model." + key] = v
        return super().load_state_dict(sd, strict=strict, **k)

    def forward(self, input_ids, attention_mask=None, position_ids=None, output_attentions=None, output_hidden_states=False,
                return_dict=True):
        if attention_mask is not None:
            raise ValueError("CLIPTextModel (libctrlhip): attention_mask is not supported (the reference passes None, "
                             "model/ctrl_helper.py:362)")
        if position_ids is not None or output_attentions:
            raise ValueError("CLIPTextModel (libctrlhip): position_ids / output_attentions are not supported")
        dev = self.device
        if not dev.type == "cuda":
            raise RuntimeError("parameters must live on the GPU before the first forward (call .to('cuda')); there is no CPU path")
        ids = input_ids
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.is_floating_point():
            raise ValueError("input_ids must be an integer tensor [batch, tokens]")
        N, Lt = ids.shape
        if Lt < 1 or Lt > self.config.max_position_embeddings:
            raise ValueError("input_ids: %d tokens (1 .. %d)" % (Lt, self.config.max_position_embeddings))
        on_host = not ids.is_cuda
        if on_host and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.config.vocab_size):
            raise ValueError("input_ids hold ids outside the vocabulary [0, %d)" % self.config.vocab_size)
        ids = ids.to(device=dev, dtype=torch.int64).contiguous()
        dt = self.dtype
        Cn = self.config.hidden_size
        last = torch.empty((N, Lt, Cn), dtype=dt, device=dev)
        pooled = torch.empty((N, Cn), dtype=dt, device=dev)
        hid = torch.empty((self.config.num_hidden_layers + 1, N, Lt, Cn), dtype=dt, device=dev) if output_hidden_states else None
        with torch.cuda.device(dev):
            plan = self._ensure_plan()
            L.check(L.lib().ctrl_text_encoder_forward(plan, L.ptr(ids), N, Lt, L.ptr(last), L.ptr(pooled), L.ptr(hid),
                                                      L.dtype_code(dt), L.cur_stream()))
            if not on_host and not torch.cuda.is_current_stream_capturing():
                if L.lib().ctrl_text_encoder_id_status(plan, 1) != 0:
                    raise ValueError("input_ids hold ids outside the vocabulary [0, %d) (they were clamped)" % self.config.vocab_size)
        L.raise_if_out_of_range("CLIPTextModel")
        hs = tuple(hid.unbind(0)) if hid is not None else None
        if not return_dict:
            return (last, pooled) + ((hs,) if hs is not None else ())
        return CLIPTextOutput(last, pooled, hs)


def _check_ids_in_vocab(ids, text_encoder):
    vocab = getattr(getattr(text_encoder, "config", None), "vocab_size", None)
    if vocab is not None and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise ValueError("the tokenizer produced ids outside the text encoder's vocabulary [0, %d)" % vocab)


@torch.no_grad()
def encode_controlnet_prompt(tokenizer, text_encoder, prompt, device, num_images_per_prompt, do_classifier_free_guidance,
                             negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
    """ControlNetHelper.encode_controlnet_prompt (model/ctrl_helper.py:300-457) with the tokenizer and the text encoder passed in.
    Returns (prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds).

    The prompts and the negative prompts go through ONE encoder forward (with clip_skip, the prompt rows take final_layer_norm of
    hidden state -(clip_skip + 1) and the negative rows the last hidden state, as in the reference's two calls).  Uses only the
    encoder's module interface (`__call__`, `.dtype`, `.config`, `.text_model.final_layer_norm`).  Deviation: where the reference
    raises UnboundLocalError -- no classifier-free guidance, or `prompt_embeds` / `negative_prompt_embeds` given -- the values it
    never assigns are returned as None.  `lora_scale` is accepted and ignored, as in the reference."""
    del lora_scale
    if prompt is not None and isinstance(prompt, str):
        batch_size = 1
    elif prompt is not None and isinstance(prompt, list):
        batch_size = len(prompt)
    else:
        batch_size = prompt_embeds.shape[0]

    # the negative tokens (model/ctrl_helper.py:396-416), checked before anything runs
    uncond_tokens = None
    if do_classifier_free_guidance and negative_prompt_embeds is None:
        if negative_prompt is None:
            uncond_tokens = [""] * batch_size
        elif prompt is not None and type(prompt) is not type(negative_prompt):
            raise TypeError("`negative_prompt` should be the same type to `prompt`, but got %s != %s." % (type(negative_prompt), type(prompt)))
        elif isinstance(negative_prompt, str):
            uncond_tokens = [negative_prompt]
        elif batch_size != len(negative_prompt):
            raise ValueError("`negative_prompt`: %s has batch size %d, but `prompt`: %s has batch size %d. Please make sure that passed "
                             "`negative_prompt` matches the batch size of `prompt`." % (negative_prompt, len(negative_prompt), prompt, batch_size))
        else:
            uncond_tokens = negative_prompt

    def tokenize(texts, max_length):
        ids = tokenizer(texts, padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids
        _check_ids_in_vocab(ids, text_encoder)
        return ids

    pooled_prompt_embeds = negative_pooled_prompt_embeds = None
    neg_out = None
    if prompt_embeds is None:
        ids = tokenize(prompt, tokenizer.model_max_length)
        n_pos = ids.shape[0]
        if uncond_tokens is not None:
            uids = tokenize(uncond_tokens, ids.shape[1])
            ids = torch.cat([ids, uids], 0)
        out = text_encoder(ids.to(device), attention_mask=None, output_hidden_states=clip_skip is not None)
        if clip_skip is None:
            prompt_embeds = out[0][:n_pos]
        else:
            prompt_embeds = text_encoder.text_model.final_layer_norm(out[-1][-(clip_skip + 1)][:n_pos])
        pooled_prompt_embeds = out[1][:n_pos]
        if uncond_tokens is not None:
            neg_out = (out[0][n_pos:], out[1][n_pos:])

    prompt_embeds_dtype = text_encoder.dtype if text_encoder is not None else prompt_embeds.dtype
    prompt_embeds = prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)
    bs_embed, seq_len, _ = prompt_embeds.shape
    prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)

    if uncond_tokens is not None and neg_out is None:          # prompt_embeds were given: the negatives alone
        uids = tokenize(uncond_tokens, seq_len)
        o = text_encoder(uids.to(device), attention_mask=None)
        neg_out = (o[0], o[1])
    if neg_out is not None:
        negative_prompt_embeds, negative_pooled_prompt_embeds = neg_out

    if pooled_prompt_embeds is not None:
        pooled_prompt_embeds = pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)

    if do_classifier_free_guidance:
        seq_len = negative_prompt_embeds.shape[1]
        negative_prompt_embeds = negative_prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)
        negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
        if negative_pooled_prompt_embeds is not None:
            negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)

    return prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds


# ------------------------------------------------------------------------------------------ SDXL: OpenCLIP bigG + encode_prompt
class CLIPTextModelOutput(tuple):
    """(text_embeds, last_hidden_state[, hidden_states]) with attribute access, indexed like transformers' CLIPTextModelOutput"""

    def __new__(cls, text_embeds, last_hidden_state, hidden_states=None):
        items = (text_embeds, last_hidden_state) + ((hidden_states,) if hidden_states is not None else ())
        self = super().__new__(cls, items)
        self.text_embeds, self.last_hidden_state, self.hidden_states = text_embeds, last_hidden_state, hidden_states
        return self


def _forward_ext(model, ids, last=False, pooled=False, embeds=False, hidden_index=None):
    """one ctrl_text_encoder_forward_ext of a mirror (CLIPTextModel or CLIPTextModelWithProjection) over int64 ids [N][L]:
    returns (last, pooled, embeds, hidden) in the model's dtype, None where not asked; hidden_index None = no state, -1 = all
    [layers + 1][N][L][C], k = state k [N][L][C] (with no last / pooled / embeds the layers after k are not run)"""
    dev = model.device
    if dev.type != "cuda":
        raise RuntimeError("parameters must live on the GPU before the first forward (call .to('cuda')); there is no CPU path")
    if ids.dim() != 2 or ids.is_floating_point():
        raise ValueError("input_ids must be an integer tensor [batch, tokens]")
    N, Lt = ids.shape
    cfg = model.config
    if Lt < 1 or Lt > cfg.max_position_embeddings:
        raise ValueError("input_ids: %d tokens (1 .. %d)" % (Lt, cfg.max_position_embeddings))
    on_host = not ids.is_cuda
    if on_host and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size):
        raise ValueError("input_ids hold ids outside the vocabulary [0, %d)" % cfg.vocab_size)
    ids = ids.to(device=dev, dtype=torch.int64).contiguous()
    dt, Cn = model.dtype, cfg.hidden_size
    o_last = torch.empty((N, Lt, Cn), dtype=dt, device=dev) if last else None
    o_pool = torch.empty((N, Cn), dtype=dt, device=dev) if pooled else None
    o_emb = torch.empty((N, cfg.projection_dim), dtype=dt, device=dev) if embeds else None
    hid = None
    if hidden_index is not None:
        shape = (cfg.num_hidden_layers + 1, N, Lt, Cn) if hidden_index < 0 else (N, Lt, Cn)
        hid = torch.empty(shape, dtype=dt, device=dev)
    with torch.cuda.device(dev):
        plan = model._ensure_plan()
        L.check(L.lib().ctrl_text_encoder_forward_ext(plan, L.ptr(ids), N, Lt, L.ptr(o_last), L.ptr(o_pool), L.ptr(o_emb), L.ptr(hid),
                                                      -1 if hidden_index is None else int(hidden_index), L.dtype_code(dt),
                                                      L.cur_stream()))
        if not on_host and not torch.cuda.is_current_stream_capturing():
            if L.lib().ctrl_text_encoder_id_status(plan, 1) != 0:
                raise ValueError("input_ids hold ids outside the vocabulary [0, %d) (they were clamped)" % cfg.vocab_size)
    L.raise_if_out_of_range(type(model).__name__)
    return o_last, o_pool, o_emb, hid


class CLIPTextModelWithProjection(ParamTreeModule):
    """Drop-in mirror of transformers' CLIPTextModelWithProjection (SDXL's `text_encoder_2`, OpenCLIP ViT-bigG: hidden 1280, 20 heads,
    intermediate 5120, 32 layers, exact gelu, a bias-free text_projection) whose forward runs in libctrlhip (ctrl_text_encoder_create_ext).
    Weights: the `text_model.*` keys and `text_projection.weight` (the prefix-less text-model keys load as well).  `gemm_form` picks
    the GEMM of the plan (0: the pinned implicit GEMM, the default; 1: the few-row GEMM of csrc/text_gemm.hip, opt-in: faster at
    B = 1, even at B = 2 and 2.4x slower at B = 16, profiles/sdxl_text_encoder_bench.txt); both are batch-invariant."""

    GEMM_FORM = 0
    _CREATE, _DESTROY, _CREATE_CFG = "ctrl_text_encoder_create_ext", "ctrl_text_encoder_destroy", ("_cfg", "_ext")

    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                 num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                 attention_dropout=0.0, initializer_range=0.02, initializer_factor=1.0, pad_token_id=1, bos_token_id=49406,
                 eos_token_id=49407, gemm_form=None, **unused):
        super().__init__()
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__", "unused", "gemm_form")})
        unsupported = []
        if hidden_act not in ("quick_gelu", "gelu"):
            unsupported.append("hidden_act %r (quick_gelu or gelu)" % (hidden_act,))
        if num_attention_heads < 1 or hidden_size != 64 * num_attention_heads:
            unsupported.append("head_dim %s (64 only)" % (hidden_size / max(num_attention_heads, 1)))
        if max_position_embeddings > 77:
            unsupported.append("max_position_embeddings %d (<= 77)" % max_position_embeddings)
        if hidden_size > 2048 or intermediate_size % 64:
            unsupported.append("hidden_size > 2048 or intermediate_size not a multiple of 64")
        if projection_dim < 1:
            unsupported.append("projection_dim %d (>= 1)" % projection_dim)
        if unsupported:
            raise ValueError("CLIPTextModelWithProjection (libctrlhip): unsupported configuration: " + ", ".join(unsupported))
        cfg = L.TextEncoderConfig()
        cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = vocab_size, hidden_size, intermediate_size
        cfg.num_hidden_layers, cfg.num_attention_heads = num_hidden_layers, num_attention_heads
        cfg.max_position_embeddings, cfg.eos_token_id, cfg.layer_norm_eps = max_position_embeddings, eos_token_id, layer_norm_eps
        self._cfg = cfg
        ext = L.TextEncoderExt()
        ext.hidden_act = 1 if hidden_act == "gelu" else 0
        ext.projection_dim = projection_dim
        ext.gemm_form = self.GEMM_FORM if gemm_form is None else int(gemm_form)
        self._ext = ext
        self.add_module("text_model", nn.Module())
        self.text_model.add_module("final_layer_norm", _FinalLayerNorm(layer_norm_eps))
        spec = text_encoder_spec(vocab_size, hidden_size, intermediate_size, num_hidden_layers, max_position_embeddings)
        self._register_spec(spec + [("text_projection.weight", (projection_dim, hidden_size))], dtype=torch.float32)

    @property
    def gemm_form(self):
        return self._ext.gemm_form

    def config_dict(self):
        return dict(self.config, architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model")

    def save_pretrained(self, path, safe_serialization=True, variant=None, **unused):
        """transformers' layout: config.json + model[.variant].safetensors"""
        import json
        import os
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as fh:
            json.dump(self.config_dict(), fh, indent=2)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        stem = "model" + (".%s" % variant if variant else "")
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, os.path.join(path, stem + ".safetensors"))
        else:
            torch.save(sd, os.path.join(path, stem + ".bin"))

    def load_state_dict(self, state_dict, strict=True, **k):
        """the transformers keys (`text_model.` prefix + `text_projection.weight`) or the text-model keys without the prefix; the
        non-persistent `position_ids` buffer some checkpoints carry is dropped"""
        sd = {}
        for key, v in state_dict.items():
            if key.endswith("embeddings.position_ids"):
                continue
            sd[key if key.startswith(("text_model.", "text_projection.")) else "text_model." + key] = v
        return super().load_state_dict(sd, strict=strict, **k)

    def forward(self, input_ids, attention_mask=None, position_ids=None, output_attentions=None, output_hidden_states=False,
                return_dict=True):
        if attention_mask is not None:
            raise ValueError("CLIPTextModelWithProjection (libctrlhip): attention_mask is not supported (the SDXL pipeline passes none)")
        if position_ids is not None or output_attentions:
            raise ValueError("CLIPTextModelWithProjection (libctrlhip): position_ids / output_attentions are not supported")
        ids = input_ids[None] if input_ids.dim() == 1 else input_ids
        last, _, emb, hid = _forward_ext(self, ids, last=True, embeds=True, hidden_index=-1 if output_hidden_states else None)
        hs = tuple(hid.unbind(0)) if hid is not None else None
        if not return_dict:
            return (emb, last) + ((hs,) if hs is not None else ())
        return CLIPTextModelOutput(emb, last, hs)


def _is_mirror(enc):
    return isinstance(enc, (CLIPTextModel, CLIPTextModelWithProjection))


def _encode_states(enc, ids, pos_index, neg_index, n_pos, want_pooled):
    """one forward of `enc` over ids (positives first, then negatives): the positive rows' hidden state pos_index, the negative rows'
    state neg_index (negative indices as in transformers' tuple) and, when asked, out[0] (what the SDXL method takes as pooled)"""
    layers = enc.config.num_hidden_layers
    if _is_mirror(enc):
        pi, ni = pos_index % (layers + 1), neg_index % (layers + 1)
        proj = isinstance(enc, CLIPTextModelWithProjection)
        one = pi == ni or n_pos == ids.shape[0]
        o_last, _, emb, hid = _forward_ext(enc, ids, last=want_pooled and not proj, embeds=want_pooled and proj,
                                           hidden_index=pi if one else -1)
        pos, neg = (hid[:n_pos], hid[n_pos:]) if one else (hid[pi][:n_pos], hid[ni][n_pos:])
        return pos, neg, ((emb if proj else o_last) if want_pooled else None)
    out = enc(ids, output_hidden_states=True)
    hs = out.hidden_states if hasattr(out, "hidden_states") else out[-1]
    return hs[pos_index][:n_pos], hs[neg_index][n_pos:], out[0]


@torch.no_grad()
def encode_sdxl_prompt(tokenizers, text_encoders, prompt, prompt_2=None, device=None, num_images_per_prompt=1,
                       do_classifier_free_guidance=True, negative_prompt=None, negative_prompt_2=None, prompt_embeds=None,
                       negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, lora_scale=None,
                       clip_skip=None, force_zeros_for_empty_prompt=True):
    """The SDXL pipeline's encode_prompt (sdxl/pipelines/sdxl_controlnet_adapter_pipeline.py:282-515) with the tokenizers and text
    encoders passed in ([tokenizer, tokenizer_2] / [text_encoder, text_encoder_2], or the second alone).  Returns (prompt_embeds,
    negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds), the method's values.

    Each encoder runs ONE forward over the prompts and the negative prompts together (batch invariance makes the rows bit-identical
    to the method's separate calls).  On the libctrlhip mirrors it runs ctrl_text_encoder_forward_ext and writes only the hidden state
    it needs (the CLIP-L tower stops after its penultimate layer); other encoders are called as modules with output_hidden_states=True.
    Deviations: `lora_scale` and textual inversion are accepted and ignored; the truncation warning is not logged."""
    del lora_scale
    prompt = [prompt] if isinstance(prompt, str) else prompt
    if prompt is not None:
        batch_size = len(prompt)
    else:
        batch_size = prompt_embeds.shape[0]
    tokenizers, text_encoders = list(tokenizers), list(text_encoders)

    zero_out_negative_prompt = negative_prompt is None and force_zeros_for_empty_prompt
    uncond = None
    if do_classifier_free_guidance and negative_prompt_embeds is None and not zero_out_negative_prompt:
        negative_prompt = negative_prompt or ""
        negative_prompt_2 = negative_prompt_2 or negative_prompt
        negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
        if prompt is not None and type(prompt) is not type(negative_prompt):
            raise TypeError("`negative_prompt` should be the same type to `prompt`, but got %s != %s." % (type(negative_prompt), type(prompt)))
        elif batch_size != len(negative_prompt):
            raise ValueError("`negative_prompt`: %s has batch size %d, but `prompt`: %s has batch size %d. Please make sure that passed "
                             "`negative_prompt` matches the batch size of `prompt`." % (negative_prompt, len(negative_prompt), prompt, batch_size))
        uncond = [negative_prompt, negative_prompt_2]

    def tokenize(tok, enc, texts, max_length):
        ids = tok(texts, padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids
        _check_ids_in_vocab(ids, enc)
        return ids

    pos_index = -2 if clip_skip is None else -(clip_skip + 2)
    neg_list = []
    if prompt_embeds is None:
        prompt_2 = prompt_2 or prompt
        prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
        pos_list = []
        for i, (p, tok, enc) in enumerate(zip([prompt, prompt_2], tokenizers, text_encoders)):
            ids = tokenize(tok, enc, p, tok.model_max_length)
            n_pos = ids.shape[0]
            if uncond is not None:          # the method tokenizes the negatives to prompt_embeds.shape[1] (= the positives' length)
                ids = torch.cat([ids, tokenize(tok, enc, uncond[i], ids.shape[1])], 0)
            last_enc = i == len(text_encoders) - 1
            pos, neg, pooled = _encode_states(enc, ids.to(device), pos_index, -2, n_pos, want_pooled=last_enc)
            pos_list.append(pos)
            if uncond is not None:
                neg_list.append(neg)
            if last_enc:
                pooled_prompt_embeds = pooled[:n_pos]
                if uncond is not None:
                    negative_pooled_prompt_embeds = pooled[n_pos:]
        prompt_embeds = torch.concat(pos_list, dim=-1)
    elif uncond is not None:                # prompt_embeds given: the negatives alone
        for i, (tok, enc) in enumerate(zip(tokenizers, text_encoders)):
            ids = tokenize(tok, enc, uncond[i], prompt_embeds.shape[1])
            _, neg, pooled = _encode_states(enc, ids.to(device), -2, -2, 0, want_pooled=i == len(text_encoders) - 1)
            neg_list.append(neg)
            if pooled is not None:
                negative_pooled_prompt_embeds = pooled

    if do_classifier_free_guidance and negative_prompt_embeds is None and zero_out_negative_prompt:
        negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
    elif uncond is not None:
        negative_prompt_embeds = torch.concat(neg_list, dim=-1)

    dtype = text_encoders[-1].dtype
    prompt_embeds = prompt_embeds.to(dtype=dtype, device=device)
    bs_embed, seq_len, _ = prompt_embeds.shape
    prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)
    if do_classifier_free_guidance:
        seq_len = negative_prompt_embeds.shape[1]
        negative_prompt_embeds = negative_prompt_embeds.to(dtype=dtype, device=device)
        negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
    pooled_prompt_embeds = pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)
    if do_classifier_free_guidance:
        negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.repeat(1, num_images_per_prompt).view(bs_embed * num_images_per_prompt, -1)
    return prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds
