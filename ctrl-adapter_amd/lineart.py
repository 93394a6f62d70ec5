"""LineartDetector / extract_lineart -- controlnet_aux's lineart annotator on libctrlhip: the detector the reference makes its `lineart`
condition with.

`add_lineart_estimator` (model/ctrl_helper.py:111-114) builds `LineartDetector.from_pretrained('lllyasviel/Annotators')`;
`prepare_conditioning_images` (190-191) calls it once per frame.  Here a clip's frames go to the GPU once: the stem and head kernels, the
InstanceNorm statistics / apply kernels of csrc/lineart.hip and nine convolutions on the implicit GEMM (csrc/plan_lineart.cpp) give the
uint8 maps, which stay on the device as [N, H, W, 3], slices of which `prepare_images` takes as they are.  No CPU fallback.

controlnet_aux is not installed where this was written, so the network is restated from knowledge (tests/test_lineart_host.py pins the layer
semantics against torch's own layers and keeps the pin to controlnet_aux itself as a skipped test).  LineartDetector holds two
`Generator(3, 1, 3)` instances, sk_model.pth and -- for coarse=True -- sk_model2.pth; norm_layer = nn.InstanceNorm2d: no affine
parameters, no running statistics, eps 1e-5, biased variance:

    model0   ReflectionPad2d(3), Conv2d(3, 64, 7), IN, ReLU
    model1   Conv2d(64, 128, 3, stride 2, padding 1), IN, ReLU; Conv2d(128, 256, 3, stride 2, padding 1), IN, ReLU
    model2   three blocks x + [ReflectionPad2d(1), Conv2d(256, 256, 3), IN, ReLU, ReflectionPad2d(1), Conv2d(256, 256, 3), IN]
    model3   ConvTranspose2d(256, 128, 3, stride 2, padding 1, output_padding 1), IN, ReLU; ConvTranspose2d(128, 64, ...), IN, ReLU
    model4   ReflectionPad2d(3), Conv2d(64, 1, 7), Sigmoid

`__call__`: HWC3 and resize_image; RGB / 255 as 1 c h w (no BGR flip); line = model(image)[0][0]; (line * 255).clip(0, 255).astype(uint8)
(truncation); HWC3 and resize; 255 - map.

Sizes: only inputs that controlnet_aux's `resize_image` would leave unchanged run -- H and W multiples of 64 and
min(H, W) == detect_resolution == image_resolution (the reference's 512 x 512 frames); anything else raises ValueError.

A bias in front of an affine-free InstanceNorm cancels, so the plan drops every bias but model4.1's; the state-dict check still wants
them present and well-shaped.  A forward in which an activation leaves the fp16 range raises RuntimeError instead of returning a wrong
map.  The real checkpoints' activation ranges are not known here (sk_model.pth and sk_model2.pth have not been run); every convolution's
output is normalised to unit variance per channel before it is stored again, which keeps the stored activations small.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from .hed import _as_u8_rgb


def lineart_state_dict_spec():
    """(name, shape) of every parameter of controlnet_aux's lineart Generator(3, 1, 3)"""
    spec = []

    def both(name, wshape):
        spec.append((name + ".weight", wshape))
        spec.append((name + ".bias", (wshape[1] if name.startswith("model3.") else wshape[0],)))

    both("model0.1", (64, 3, 7, 7))
    both("model1.0", (128, 64, 3, 3))
    both("model1.3", (256, 128, 3, 3))
    for b in range(3):
        for j in (1, 5):
            both("model2.%d.conv_block.%d" % (b, j), (256, 256, 3, 3))
    both("model3.0", (256, 128, 3, 3))          # ConvTranspose2d: [Cin][Cout][3][3]
    both("model3.3", (128, 64, 3, 3))
    both("model4.1", (1, 64, 7, 7))
    return spec


def _load_local(local_path, filename, who, required=True):
    path = str(local_path)
    if os.path.isdir(path):
        tried = [os.path.join(path, filename), os.path.join(path, "annotator", "ckpts", filename)]
        path = next((p for p in tried if os.path.exists(p)), None)
        if path is None:
            if not required:
                return None
            raise FileNotFoundError("%s: no %s under %s (local files only; nothing is downloaded)" % (who, filename, local_path))
    elif not os.path.exists(path):
        raise FileNotFoundError("%s: %s does not exist (local files only; nothing is downloaded)" % (who, path))
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    return ckpt["state_dict"] if "state_dict" in ckpt else ckpt


class LineartDetector:
    """controlnet_aux.LineartDetector over a libctrlhip plan.  `LineartDetector.from_state_dict(sd, sd_coarse=None)` takes the state dicts
    of the fine and (optionally) the coarse Generator, `LineartDetector.from_pretrained(dir)` a local directory holding sk_model.pth (and
    sk_model2.pth)."""

    def __init__(self, state_dict, state_dict_coarse=None, device=None, ws_cap_bytes=0):
        checked = {}                 # (the state dicts are checked first: a wrong checkpoint is refused with or without a GPU)
        for prefix, sd in (("fine.", state_dict), ("coarse.", state_dict_coarse)):
            if sd is None:
                continue
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
            for name, shape in lineart_state_dict_spec():
                if name not in sd:
                    raise KeyError("LineartDetector: the %s state dict has no %r (Generator(3, 1, 3)'s keys are expected)" % (prefix[:-1], name))
                v = sd[name]
                if tuple(v.shape) != tuple(shape):
                    raise ValueError("LineartDetector: %s%s has shape %s, expected %s" % (prefix, name, tuple(v.shape), tuple(shape)))
                checked[prefix + name] = v
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        device = torch.device(device) if device is not None else None
        if device is None or device.type != "cuda":
            raise RuntimeError("LineartDetector (libctrlhip) runs on the GPU only; there is no CPU fallback")
        self.device = device
        self.has_coarse = state_dict_coarse is not None
        self._params = {k: v.detach().to(device=device, dtype=torch.float32).contiguous() for k, v in checked.items()}
        self._cfg = L.LineartConfig(0, int(self.has_coarse), int(ws_cap_bytes))
        self._plan = None
        refs = (L.TensorRef * len(self._params))()
        keep = []
        for i, (k, t) in enumerate(self._params.items()):
            kb = k.encode()
            keep.append(kb)
            refs[i].name = kb
            refs[i].data = t.data_ptr()
            refs[i].dtype = L.F32
            refs[i].ndim = t.dim()
            for d in range(t.dim()):
                refs[i].shape[d] = t.shape[d]
        h = C.c_void_p()
        with torch.cuda.device(device):
            L.check(L.lib().ctrl_lineart_create(C.byref(self._cfg), refs, len(self._params), L.cur_stream(), C.byref(h)))
        self._plan = h

    @classmethod
    def from_state_dict(cls, sd, sd_coarse=None, **kw):
        return cls(sd, sd_coarse, **kw)

    @classmethod
    def from_pretrained(cls, local_dir, filename="sk_model.pth", coarse_filename="sk_model2.pth", **kw):
        """loads LOCAL checkpoints (a directory holding `filename`, also under annotator/ckpts, or the fine checkpoint's file); nothing is
        downloaded.  The coarse generator is loaded when `coarse_filename` lies beside it; without it coarse=True raises ValueError."""
        who = "LineartDetector.from_pretrained"
        fine = _load_local(local_dir, filename, who)
        base = str(local_dir) if os.path.isdir(str(local_dir)) else os.path.dirname(str(local_dir))
        coarse = _load_local(base, coarse_filename, who, required=False) if os.path.isdir(base) else None
        return cls(fine, coarse, **kw)

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None:
                L.lib().ctrl_lineart_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    def to(self, device):
        """controlnet_aux's `.to("cuda")` (model/ctrl_helper.py:114): the plan already lives on its GPU; another device is refused"""
        d = torch.device(device)
        if d.type != self.device.type or (d.index is not None and d.index != self.device.index):
            raise ValueError("LineartDetector: the plan lives on %s; create another detector for %s" % (self.device, device))
        return self

    def workspace_bytes(self, N, H, W, frames_per_group=None):
        return int(L.lib().ctrl_lineart_ws_bytes(self._plan, int(N), int(H), int(W), int(frames_per_group or 0)))

    @torch.no_grad()
    def run(self, frames, coarse=False, channels=3, frames_per_group=None, return_logits=False):
        """frames uint8 [N, H, W, 3] (RGB) on the detector's GPU -> uint8 [N, H, W, 3] (channels=3) or [N, H, W]; with return_logits also the
        fp32 [N, H, W] output of model4.1 in front of the sigmoid"""
        if channels not in (1, 3):
            raise ValueError("LineartDetector: channels must be 1 or 3")
        if coarse and not self.has_coarse:
            raise ValueError("LineartDetector: coarse=True needs the coarse generator (sk_model2.pth), which this detector was created without")
        if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError("LineartDetector.run: frames must be a uint8 tensor [N, H, W, 3]")
        if frames.device != self.device:
            raise ValueError("LineartDetector.run: frames live on %s, the detector on %s" % (frames.device, self.device))
        fpg = 0 if frames_per_group is None else int(frames_per_group)
        if frames_per_group is not None and fpg < 1:
            raise ValueError("frames_per_group must be None or positive (got %r)" % (frames_per_group,))
        frames = frames.contiguous()
        N, H, W = frames.shape[:3]
        if N < 1 or H % 64 or W % 64 or H < 64 or W < 64:
            raise ValueError("LineartDetector: %d frames of %d x %d: at least one frame with H and W multiples of 64 is required (the sizes "
                             "controlnet_aux's resize_image produces)" % (N, H, W))
        out = torch.empty((N, H, W, 3) if channels == 3 else (N, H, W), dtype=torch.uint8, device=self.device)
        logits = torch.empty((N, H, W), dtype=torch.float32, device=self.device) if return_logits else None
        with torch.cuda.device(self.device):
            L.check(L.lib().ctrl_lineart_forward(self._plan, L.ptr(frames), N, H, W, int(bool(coarse)), channels, L.ptr(out), L.ptr(logits), fpg,
                                                 L.cur_stream()))
        return (out, logits) if return_logits else out

    def __call__(self, input_image, coarse=False, detect_resolution=512, image_resolution=512, output_type="pil", frames_per_group=None):
        """controlnet_aux.LineartDetector.__call__ for one image or a list of frames of one size.  output_type "pil": a PIL image (a list
        for a list), "np": uint8 arrays, "pt": ONE uint8 tensor [N, H, W, 3] that stays on the GPU (what prepare_images takes)."""
        if output_type not in ("pil", "np", "pt"):
            raise ValueError("LineartDetector: output_type must be 'pil', 'np' or 'pt'")
        if coarse and not self.has_coarse:
            raise ValueError("LineartDetector: coarse=True needs the coarse generator (sk_model2.pth), which this detector was created without")
        single = not isinstance(input_image, (list, tuple)) and not (torch.is_tensor(input_image) and input_image.dim() == 4)
        images = [input_image] if single else list(input_image)
        try:
            frames = [_as_u8_rgb(i) for i in images]
        except ValueError as e:
            raise ValueError(str(e).replace("HEDdetector", "LineartDetector")) from None
        if not frames or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("LineartDetector needs at least one image and all images of one size")
        H, W = frames[0].shape[:2]
        if H % 64 or W % 64 or min(H, W) != int(detect_resolution) or min(H, W) != int(image_resolution):
            raise ValueError("LineartDetector: a %d x %d image with detect_resolution=%s, image_resolution=%s would be resized by "
                             "controlnet_aux (INTER_AREA / LANCZOS4), which this library does not do: H and W must be multiples of 64 and "
                             "min(H, W) == detect_resolution == image_resolution" % (H, W, detect_resolution, image_resolution))
        src = torch.stack([f.to(self.device) for f in frames]).contiguous()
        out = self.run(src, coarse=coarse, channels=3, frames_per_group=frames_per_group)
        if output_type == "pt":
            return out
        host = out.cpu().numpy()
        if output_type == "pil":
            from PIL import Image
            res = [Image.fromarray(host[i]) for i in range(host.shape[0])]
        else:
            res = [host[i] for i in range(host.shape[0])]
        return res[0] if single else res


def extract_lineart(frames, detector, coarse=False, as_pil=False):
    """the `control_type == 'lineart'` branch of ControlNetHelper.prepare_conditioning_images (model/ctrl_helper.py:190-191:
    LineartDetector(img) per frame) for a whole clip -> uint8 [N, H, W, 3] on the GPU, or the list of PIL images"""
    if not isinstance(detector, LineartDetector):
        raise TypeError("a ctrl_adapter_amd.LineartDetector is required (there is no CPU fallback)")
    frames = list(frames)
    first = _as_u8_rgb(frames[0]) if frames else None
    res = min(first.shape[:2]) if first is not None else 512
    return detector(frames, coarse=coarse, detect_resolution=res, image_resolution=res, output_type="pil" if as_pil else "pt")
