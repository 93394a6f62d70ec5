"""CLIPVisionModelWithProjection -- drop-in mirror of the image encoder of the video routes (transformers
CLIPVisionModelWithProjection: the `image_encoder` of stabilityai/stable-video-diffusion-img2vid(-xt) and ali-vilab/i2vgen-xl, CLIP
ViT-H/14) whose forward runs in libctrlhip (csrc/vision.hip, csrc/plan_vision.cpp), and the two pipelines' _encode_image:

  encode_svd_image     svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212, with _resize_with_antialiasing (:807-900), the
                       rescale and the CLIP normalisation in one GPU kernel (ctrl_op_clip_resize_aa)
  encode_i2vgen_image  i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:366-396; on the mirror the CLIP normalisation of a
                       PIL image runs inside the patch kernel (ctrl_op_vision_patchify)

State-dict keys are transformers' (`vision_model.embeddings.class_embedding`, ..., `visual_projection.weight`)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._plan import Config, ParamTreeModule, _check_gpu_input, c_spec

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
SVD_IMAGE_SIZE = 224           # the size the SVD pipeline resizes to (_encode_image: _resize_with_antialiasing(image, (224, 224)))


class CLIPVisionModelOutput(tuple):
    """(image_embeds, last_hidden_state[, hidden_states]) with attribute access, indexed like transformers' CLIPVisionModelOutput"""

    def __new__(cls, image_embeds, last_hidden_state, hidden_states=None):
        items = (image_embeds, last_hidden_state) + ((hidden_states,) if hidden_states is not None else ())
        self = super().__new__(cls, items)
        self.image_embeds, self.last_hidden_state, self.hidden_states = image_embeds, last_hidden_state, hidden_states
        return self


def _vision_config(image_size, patch_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, projection_dim,
                   hidden_act, layer_norm_eps, gemm_form):
    cfg = L.VisionEncoderConfig()
    cfg.image_size, cfg.patch_size, cfg.hidden_size, cfg.intermediate_size = image_size, patch_size, hidden_size, intermediate_size
    cfg.num_hidden_layers, cfg.num_attention_heads, cfg.projection_dim = num_hidden_layers, num_attention_heads, projection_dim
    cfg.hidden_act = 1 if hidden_act == "gelu" else 0
    cfg.layer_norm_eps, cfg.gemm_form = layer_norm_eps, gemm_form
    return cfg


def vision_encoder_spec(cfg):
    """(name, shape) of every parameter of a ctrl_vision_encoder_config, from the library's inventory"""
    lib = L.lib()
    return c_spec(lib.ctrl_vision_encoder_param_count, lib.ctrl_vision_encoder_param_spec, cfg)


def _mean_std(feature_extractor, device=None):
    """(mean[3], std[3]) of a CLIPImageProcessor, the OpenAI CLIP constants when there is none"""
    mean = getattr(feature_extractor, "image_mean", None) if feature_extractor is not None else None
    std = getattr(feature_extractor, "image_std", None) if feature_extractor is not None else None
    mean = tuple(float(v) for v in (mean if mean is not None else OPENAI_CLIP_MEAN))
    std = tuple(float(v) for v in (std if std is not None else OPENAI_CLIP_STD))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("image_mean / image_std must hold three values")
    return mean, std


def _c_mean_std(mean_std):
    if mean_std is None:
        return None
    mean, std = mean_std
    return (C.c_float * 6)(*(list(mean) + list(std)))


class CLIPVisionModelWithProjection(ParamTreeModule):
    """Drop-in mirror of transformers' CLIPVisionModelWithProjection (constructor arguments of CLIPVisionConfig).  `gemm_form` picks the
    GEMM of the plan: 0 the pinned implicit GEMM (the default; profiles/vision_encoder_bench.txt), 1 the few-row split-K GEMM of
    csrc/text_gemm.hip.  Both are batch-invariant: an image's outputs are bit-identical alone or inside any batch."""

    GEMM_FORM = 0
    _CREATE, _DESTROY = "ctrl_vision_encoder_create", "ctrl_vision_encoder_destroy"

    def __init__(self, hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12,
                 num_channels=3, image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0,
                 initializer_range=0.02, initializer_factor=1.0, gemm_form=None, **unused):
        super().__init__()
        self.config = Config({k: v for k, v in locals().items() if k not in ("self", "__class__", "unused", "gemm_form")})
        unsupported = []
        if hidden_act not in ("quick_gelu", "gelu"):
            unsupported.append("hidden_act %r (quick_gelu or gelu)" % (hidden_act,))
        if num_channels != 3:
            unsupported.append("num_channels %d (3 only)" % num_channels)
        if num_attention_heads < 1 or hidden_size % num_attention_heads or hidden_size // num_attention_heads not in (40, 64, 80, 160):
            unsupported.append("head_dim %s (40, 64, 80 or 160)" % (hidden_size / max(num_attention_heads, 1)))
        if hidden_size % 64 or not 64 <= hidden_size <= 2048 or intermediate_size % 64 or intermediate_size < 64:
            unsupported.append("hidden_size / intermediate_size (multiples of 64, hidden_size <= 2048)")
        if patch_size < 1 or image_size < patch_size or image_size % patch_size or (image_size // patch_size) ** 2 + 1 > 577:
            unsupported.append("image_size %d / patch_size %d (a multiple, at most 577 tokens)" % (image_size, patch_size))
        if projection_dim < 1 or num_hidden_layers < 1:
            unsupported.append("projection_dim / num_hidden_layers (>= 1)")
        if unsupported:
            raise ValueError("CLIPVisionModelWithProjection (libctrlhip): unsupported configuration: " + ", ".join(unsupported))
        form = self.GEMM_FORM if gemm_form is None else int(gemm_form)
        if form not in (0, 1):
            raise ValueError("gemm_form must be 0 (pinned GEMM) or 1 (few-row GEMM)")
        self._cfg = _vision_config(image_size, patch_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                                   projection_dim, hidden_act, layer_norm_eps, form)
        self.tokens = (image_size // patch_size) ** 2 + 1
        self._register_spec(vision_encoder_spec(self._cfg), dtype=torch.float32)

    @property
    def gemm_form(self):
        return self._cfg.gemm_form

    def config_dict(self):
        return dict(self.config, architectures=["CLIPVisionModelWithProjection"], model_type="clip_vision_model")

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
        """transformers' keys; the non-persistent `position_ids` buffer some checkpoints carry is dropped"""
        sd = {key: v for key, v in state_dict.items() if not key.endswith("embeddings.position_ids")}
        return super().load_state_dict(sd, strict=strict, **k)

    def run(self, pixels, mean_std=None, last=False, pooled=False, embeds=True, hidden_index=None, out_dtype=None):
        """one ctrl_vision_encoder_forward: pixels on the GPU, [N][3][S][S] fp32 / fp16 / bf16 or uint8 [N][S][S][3] (read as x / 255);
        mean_std = (mean[3], std[3]) normalises them in fp32 inside the patch kernel (None: already normalised).  Returns (last, pooled,
        embeds, hidden) in out_dtype (default: the model's dtype), None where not asked; hidden_index None = no state, -1 = all
        [layers + 1][N][L][C], k = state k [N][L][C] (with nothing else asked the layers after k are not run)"""
        dev = _check_gpu_input(self, pixels, "pixel_values", "live")
        S = self.config.image_size
        if pixels.dtype == torch.uint8:
            if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (S, S, 3):
                raise ValueError("uint8 pixels must be [N, %d, %d, 3] (got %s)" % (S, S, tuple(pixels.shape)))
            pdt = L.U8_NHWC
        else:
            if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, S, S):
                raise ValueError("pixel_values must be [N, 3, %d, %d] (got %s)" % (S, S, tuple(pixels.shape)))
            pdt = L.dtype_code(pixels.dtype)
        px = pixels.contiguous()
        N = px.shape[0]
        cfg = self.config
        dt = self.dtype if out_dtype is None else out_dtype
        Cn, Lt = cfg.hidden_size, self.tokens
        o_last = torch.empty((N, Lt, Cn), dtype=dt, device=dev) if last else None
        o_pool = torch.empty((N, Cn), dtype=dt, device=dev) if pooled else None
        o_emb = torch.empty((N, cfg.projection_dim), dtype=dt, device=dev) if embeds else None
        hid = None
        if hidden_index is not None:
            shape = (cfg.num_hidden_layers + 1, N, Lt, Cn) if hidden_index < 0 else (N, Lt, Cn)
            hid = torch.empty(shape, dtype=dt, device=dev)
        if N == 0:
            return o_last, o_pool, o_emb, hid
        with torch.cuda.device(dev):
            plan = self._ensure_plan()
            L.check(L.lib().ctrl_vision_encoder_forward(plan, L.ptr(px), pdt, N, _c_mean_std(mean_std), L.ptr(o_last), L.ptr(o_pool),
                                                        L.ptr(o_emb), L.ptr(hid), -1 if hidden_index is None else int(hidden_index),
                                                        L.dtype_code(dt), L.cur_stream()))
        L.raise_if_out_of_range("CLIPVisionModelWithProjection")
        return o_last, o_pool, o_emb, hid

    def forward(self, pixel_values, output_attentions=None, output_hidden_states=False, return_dict=True, interpolate_pos_encoding=False):
        if output_attentions or interpolate_pos_encoding:
            raise ValueError("CLIPVisionModelWithProjection (libctrlhip): output_attentions / interpolate_pos_encoding are not supported")
        last, _, emb, hid = self.run(pixel_values, last=True, embeds=True, hidden_index=-1 if output_hidden_states else None)
        hs = tuple(hid.unbind(0)) if hid is not None else None
        if not return_dict:
            return (emb, last) + ((hs,) if hs is not None else ())
        return CLIPVisionModelOutput(emb, last, hs)


def clip_resize_aa(image, size=(SVD_IMAGE_SIZE, SVD_IMAGE_SIZE), mean_std=None, out_dtype=torch.float32):
    """SVD's preprocessing on the GPU (csrc/vision.hip clip_resize_aa_kernel): x * 2 - 1, _resize_with_antialiasing(x, size) (Gaussian
    blur with reflect padding, bicubic align_corners), (x + 1) / 2 and, with mean_std, (x - mean_c) / std_c.  image: uint8 [N][H][W][3]
    (read as x / 255) or fp32 / fp16 / bf16 [N][3][H][W], on the GPU.  Returns [N][3][size] in out_dtype."""
    if not image.is_cuda:
        raise RuntimeError("clip_resize_aa: the image must live on the GPU; there is no CPU path")
    if image.dim() != 4:
        raise ValueError("clip_resize_aa: image must be 4-D")
    if image.dtype == torch.uint8:
        if image.shape[3] != 3:
            raise ValueError("clip_resize_aa: uint8 images are [N, H, W, 3]")
        N, H, W = image.shape[:3]
        dt = L.U8_NHWC
    else:
        if image.shape[1] != 3:
            raise ValueError("clip_resize_aa: float images are [N, 3, H, W]")
        N, H, W = image.shape[0], image.shape[2], image.shape[3]
        dt = L.dtype_code(image.dtype)
    OH, OW = int(size[0]), int(size[1])
    x = image.contiguous()
    out = torch.empty((N, 3, OH, OW), dtype=out_dtype, device=x.device)
    if N == 0:
        return out
    with torch.cuda.device(x.device):
        L.check(L.lib().ctrl_op_clip_resize_aa(L.ptr(x), dt, N, H, W, OH, OW, _c_mean_std(mean_std), L.ptr(out), L.dtype_code(out_dtype),
                                               L.cur_stream()))
    return out


def _is_mirror(enc):
    return isinstance(enc, CLIPVisionModelWithProjection)


def _host_images(image):
    """PIL image(s) or numpy array(s) -> (uint8 NHWC numpy, None) or (None, fp32 NHWC numpy = diffusers' pil_to_numpy value)"""
    import PIL.Image
    images = image if isinstance(image, list) else [image]
    if not images:
        raise ValueError("no image given")
    arrs = []
    for im in images:
        if isinstance(im, PIL.Image.Image):
            if im.mode != "RGB":
                raise ValueError("PIL images must be RGB (got mode %r)" % im.mode)
            arrs.append(np.asarray(im))
        elif isinstance(im, np.ndarray):
            arrs.extend(list(im) if im.ndim == 4 else [im])
        else:
            raise ValueError("image must be a PIL image, a numpy array, a list of those, or a torch tensor")
    if any(a.ndim != 3 or a.shape[2] != 3 for a in arrs):
        raise ValueError("images must be H x W x 3")
    arr = np.stack(arrs)
    if arr.dtype == np.uint8:
        return np.ascontiguousarray(arr), None
    return None, arr.astype(np.float32) / 255.0        # what pil_to_numpy makes of a non-uint8 array


def _embed_normalised(image_encoder, image, mean_std, device, dtype):
    """image_encoder(normalise(image)).image_embeds; on the mirror the normalisation runs inside its patch kernel"""
    if _is_mirror(image_encoder):
        return image_encoder.run(image.to(device), mean_std=mean_std)[2]
    mean, std = mean_std
    if image.dtype == torch.uint8:
        image = image.to(device).permute(0, 3, 1, 2).float() / 255.0
    x = image.to(device)
    m = torch.tensor(mean, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return image_encoder(((x - m) / s).to(dtype=dtype)).image_embeds


def _finish(image_embeddings, num_videos_per_prompt, do_classifier_free_guidance):
    """the pipelines' tail: [N, 1, D], repeated per video (image-major), zero negatives first under CFG"""
    image_embeddings = image_embeddings.unsqueeze(1)
    bs_embed, seq_len, _ = image_embeddings.shape
    image_embeddings = image_embeddings.repeat(1, num_videos_per_prompt, 1)
    image_embeddings = image_embeddings.view(bs_embed * num_videos_per_prompt, seq_len, -1)
    if do_classifier_free_guidance:
        image_embeddings = torch.cat([torch.zeros_like(image_embeddings), image_embeddings])
    return image_embeddings


@torch.no_grad()
def encode_svd_image(image_encoder, feature_extractor, image, device, num_videos_per_prompt, do_classifier_free_guidance):
    """The SVD pipeline's _encode_image (svd/pipelines/svd_controlnet_adapter_pipeline.py:166-212) with the encoder and the feature
    extractor passed in.  PIL / numpy input: the whole preprocessing (/ 255, x * 2 - 1, _resize_with_antialiasing to 224 x 224,
    (x + 1) / 2, CLIP normalisation) runs in one GPU kernel, then `.to(dtype)` and the encoder, as in the method.  Tensor input skips
    the resize and is normalised, as the method's feature extractor does (on the mirror: inside its patch kernel)."""
    dtype = next(image_encoder.parameters()).dtype
    mean_std = _mean_std(feature_extractor)
    device = torch.device(device) if device is not None else torch.device("cuda")
    if not isinstance(image, torch.Tensor):
        u8, f32 = _host_images(image)
        src = torch.from_numpy(u8).to(device) if u8 is not None else torch.from_numpy(f32).permute(0, 3, 1, 2).contiguous().to(device)
        pixels = clip_resize_aa(src, (SVD_IMAGE_SIZE, SVD_IMAGE_SIZE), mean_std=mean_std, out_dtype=torch.float32)
        image_embeddings = image_encoder(pixels.to(device=device, dtype=dtype)).image_embeds
    else:
        image_embeddings = _embed_normalised(image_encoder, image, mean_std, device, dtype)
    return _finish(image_embeddings, num_videos_per_prompt, do_classifier_free_guidance)


@torch.no_grad()
def encode_i2vgen_image(image_encoder, feature_extractor, image, device, num_videos_per_prompt, do_classifier_free_guidance):
    """The I2VGen-XL pipeline's _encode_image (i2vgen_xl/pipelines/i2vgen_xl_controlnet_adapter_pipeline.py:366-396) with the encoder,
    the feature extractor and the guidance flag passed in.  PIL / numpy input (already _center_crop_wide / _resize_bilinear'ed by the
    caller) is normalised (/ 255, then CLIP mean / std) -- on the mirror inside its patch kernel; tensor input reaches the encoder
    un-normalised, as in the method."""
    dtype = next(image_encoder.parameters()).dtype
    device = torch.device(device) if device is not None else torch.device("cuda")
    if not isinstance(image, torch.Tensor):
        u8, f32 = _host_images(image)
        src = torch.from_numpy(u8) if u8 is not None else torch.from_numpy(f32).permute(0, 3, 1, 2).contiguous()
        image_embeddings = _embed_normalised(image_encoder, src, _mean_std(feature_extractor), device, dtype)
    else:
        image_embeddings = image_encoder(image.to(device=device, dtype=dtype)).image_embeds
    return _finish(image_embeddings, num_videos_per_prompt, do_classifier_free_guidance)
