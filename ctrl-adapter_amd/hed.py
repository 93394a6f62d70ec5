"""HEDdetector / extract_scribble / extract_softedge -- controlnet_aux's HED annotator on libctrlhip.

The reference makes its `scribble` condition with `HEDdetector(img, scribble=True)`, one frame at a time
(model/ctrl_helper.py:124-127, 196-197); with scribble=False the same detector gives the soft-edge map control_v11p_sd15_softedge was
trained on.  Here a clip's frames go to the GPU once: the VGG-16 trunk runs on the implicit GEMM (ReLU in its epilogue), the kernels
of csrc/hed.hip do the stem, the pooling and side projections, the bilinear fuse and the scribble tail, and the uint8 maps stay on the
device as [N, H, W, 3], slices of which `prepare_images` takes as they are.  No CPU fallback.

Sizes: only inputs that controlnet_aux's `resize_image` would leave unchanged run -- H and W multiples of 64 and
min(H, W) == detect_resolution == image_resolution (the reference's 512 x 512 frames); anything else raises ValueError (cv2's INTER_AREA /
LANCZOS4 resizes are not part of this library).  safe=True raises NotImplementedError: the reference never sets it.

`trunk_scale` (a power of two, default 1): the trunk runs on trunk_scale * activations (exact: the stem multiplies, the trunk biases are
multiplied, every side projection divides).  The input is 0..255, so a checkpoint's activations can be large; a forward in which one
leaves the fp16 range raises RuntimeError instead of returning a wrong map -- create the detector with a smaller trunk_scale then.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

_CHANNELS = (64, 128, 256, 512, 512)
_LAYERS = (2, 2, 3, 3, 3)


def hed_state_dict_spec():
    """(name, shape) of every parameter of controlnet_aux's ControlNetHED_Apache2"""
    spec = [("norm", (1, 3, 1, 1))]
    cin = 3
    for k, (c, n) in enumerate(zip(_CHANNELS, _LAYERS), 1):
        for j in range(n):
            spec.append(("block%d.convs.%d.weight" % (k, j), (c, cin, 3, 3)))
            spec.append(("block%d.convs.%d.bias" % (k, j), (c,)))
            cin = c
        spec.append(("block%d.projection.weight" % k, (1, c, 1, 1)))
        spec.append(("block%d.projection.bias" % k, (1,)))
    return spec


def _as_u8_rgb(img):
    """-> uint8 tensor [H, W, 3] (host or device): np.array(img) of a PIL image, HWC3 of a one-channel image"""
    if torch.is_tensor(img):
        a = img
        if a.dtype != torch.uint8 or a.dim() not in (2, 3) or (a.dim() == 3 and a.shape[2] != 3):
            raise ValueError("HEDdetector: tensor images must be uint8 [H, W, 3] or [H, W]")
    else:
        if hasattr(img, "convert") and getattr(img, "mode", None) not in ("RGB", "L"):
            raise ValueError("HEDdetector: PIL images must have mode RGB or L, not %r" % (getattr(img, "mode", None),))
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("HEDdetector: images must be PIL images (RGB or L) or uint8 [H, W, 3] / [H, W] arrays")
        a = torch.from_numpy(np.array(a, copy=True, order="C"))
    return a if a.dim() == 3 else a.unsqueeze(-1).expand(-1, -1, 3)


class HEDdetector:
    """controlnet_aux.HEDdetector over a libctrlhip plan.  `HEDdetector.from_state_dict(sd)` takes ControlNetHED_Apache2's state dict,
    `HEDdetector.from_pretrained(path)` a local ControlNetHED.pth (or the directory that holds it)."""

    def __init__(self, state_dict, device=None, trunk_scale=1.0, ws_cap_bytes=0):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        device = torch.device(device) if device is not None else None
        if device is None or device.type != "cuda":
            raise RuntimeError("HEDdetector (libctrlhip) runs on the GPU only; there is no CPU fallback")
        m, e = math.frexp(float(trunk_scale))
        if not (trunk_scale > 0 and m == 0.5):
            raise ValueError("HEDdetector: trunk_scale must be a positive power of two, not %r" % (trunk_scale,))
        self.device = device
        self.trunk_scale = float(trunk_scale)
        self._params = {}
        for name, shape in hed_state_dict_spec():
            if name not in state_dict:
                raise KeyError("HEDdetector: the state dict has no %r (ControlNetHED_Apache2's keys are expected)" % name)
            v = state_dict[name]
            if tuple(v.shape) != tuple(shape):
                raise ValueError("HEDdetector: %r has shape %s, expected %s" % (name, tuple(v.shape), tuple(shape)))
            self._params[name] = v.detach().to(device=device, dtype=torch.float32).contiguous()
        self._cfg = L.HedConfig(self.trunk_scale, 0, int(ws_cap_bytes))
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
            L.check(L.lib().ctrl_hed_create(C.byref(self._cfg), refs, len(self._params), L.cur_stream(), C.byref(h)))
        self._plan = h

    @classmethod
    def from_state_dict(cls, state_dict, **kw):
        return cls(state_dict, **kw)

    @classmethod
    def from_pretrained(cls, local_path, filename="ControlNetHED.pth", **kw):
        """loads a LOCAL checkpoint (a file, or a directory holding `filename`, also under annotator/ckpts); nothing is downloaded"""
        import os
        path = str(local_path)
        if os.path.isdir(path):
            tried = [os.path.join(path, filename), os.path.join(path, "annotator", "ckpts", filename)]
            path = next((p for p in tried if os.path.exists(p)), None)
            if path is None:
                raise FileNotFoundError("HEDdetector.from_pretrained: no %s under %s (local files only; nothing is downloaded)" % (filename, local_path))
        elif not os.path.exists(path):
            raise FileNotFoundError("HEDdetector.from_pretrained: %s does not exist (local files only; nothing is downloaded)" % path)
        return cls(torch.load(path, map_location="cpu", weights_only=True), **kw)

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None:
                L.lib().ctrl_hed_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    def to(self, device):
        """controlnet_aux's `.to("cuda")` (model/ctrl_helper.py:127): the plan already lives on its GPU; another device is refused"""
        d = torch.device(device)
        if d.type != self.device.type or (d.index is not None and d.index != self.device.index):
            raise ValueError("HEDdetector: the plan lives on %s; create another detector for %s" % (self.device, device))
        return self

    def workspace_bytes(self, N, H, W, scribble=False, frames_per_group=None):
        return int(L.lib().ctrl_hed_ws_bytes(self._plan, int(N), int(H), int(W), int(bool(scribble)), int(frames_per_group or 0)))

    @torch.no_grad()
    def run(self, frames, scribble=False, channels=3, frames_per_group=None, return_logits=False):
        """frames uint8 [N, H, W, 3] on the detector's GPU -> uint8 [N, H, W, 3] (channels=3) or [N, H, W]; with return_logits also the fp32
        [N, H, W] mean of the five resized side outputs in front of the sigmoid"""
        if channels not in (1, 3):
            raise ValueError("HEDdetector: channels must be 1 or 3")
        if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError("HEDdetector.run: frames must be a uint8 tensor [N, H, W, 3]")
        if frames.device != self.device:
            raise ValueError("HEDdetector.run: frames live on %s, the detector on %s" % (frames.device, self.device))
        fpg = 0 if frames_per_group is None else int(frames_per_group)
        if frames_per_group is not None and fpg < 1:
            raise ValueError("frames_per_group must be None or positive (got %r)" % (frames_per_group,))
        frames = frames.contiguous()
        N, H, W = frames.shape[:3]
        if N < 1 or H % 64 or W % 64 or H < 64 or W < 64:
            raise ValueError("HEDdetector: %d frames of %d x %d: at least one frame with H and W multiples of 64 is required (the sizes "
                             "controlnet_aux's resize_image produces)" % (N, H, W))
        out = torch.empty((N, H, W, 3) if channels == 3 else (N, H, W), dtype=torch.uint8, device=self.device)
        logits = torch.empty((N, H, W), dtype=torch.float32, device=self.device) if return_logits else None
        with torch.cuda.device(self.device):
            L.check(L.lib().ctrl_hed_forward(self._plan, L.ptr(frames), N, H, W, int(bool(scribble)), channels, L.ptr(out), L.ptr(logits), fpg,
                                             L.cur_stream()))
        return (out, logits) if return_logits else out

    def __call__(self, input_image, detect_resolution=512, image_resolution=512, safe=False, scribble=False, output_type="pil",
                 frames_per_group=None):
        """controlnet_aux.HEDdetector.__call__ for one image or a list of frames of one size.  output_type "pil": a PIL image (a list for a
        list), "np": uint8 arrays, "pt": ONE uint8 tensor [N, H, W, 3] that stays on the GPU (what prepare_images takes)."""
        if safe:
            raise NotImplementedError("HEDdetector: safe=True (the quantised safe_step) is not implemented; the reference never sets it")
        if output_type not in ("pil", "np", "pt"):
            raise ValueError("HEDdetector: output_type must be 'pil', 'np' or 'pt'")
        single = not isinstance(input_image, (list, tuple)) and not (torch.is_tensor(input_image) and input_image.dim() == 4)
        images = [input_image] if single else list(input_image)
        frames = [_as_u8_rgb(i) for i in images]
        if not frames or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("HEDdetector needs at least one image and all images of one size")
        H, W = frames[0].shape[:2]
        if H % 64 or W % 64 or min(H, W) != int(detect_resolution) or min(H, W) != int(image_resolution):
            raise ValueError("HEDdetector: a %d x %d image with detect_resolution=%s, image_resolution=%s would be resized by "
                             "controlnet_aux (INTER_AREA / LANCZOS4), which this library does not do: H and W must be multiples of 64 and "
                             "min(H, W) == detect_resolution == image_resolution" % (H, W, detect_resolution, image_resolution))
        src = torch.stack([f.to(self.device) for f in frames]).contiguous()
        out = self.run(src, scribble=scribble, channels=3, frames_per_group=frames_per_group)
        if output_type == "pt":
            return out
        host = out.cpu().numpy()
        if output_type == "pil":
            from PIL import Image
            res = [Image.fromarray(host[i]) for i in range(host.shape[0])]
        else:
            res = [host[i] for i in range(host.shape[0])]
        return res[0] if single else res


def _extract(frames, detector, scribble, as_pil):
    from .pidinet import PidiNetDetector
    if not isinstance(detector, (HEDdetector, PidiNetDetector)):
        raise TypeError("a ctrl_adapter_amd.HEDdetector or PidiNetDetector is required (there is no CPU fallback)")
    frames = list(frames)
    first = _as_u8_rgb(frames[0]) if frames else None
    res = min(first.shape[:2]) if first is not None else 512
    out = detector(frames, detect_resolution=res, image_resolution=res, scribble=scribble, output_type="pil" if as_pil else "pt")
    return out


def extract_scribble(frames, detector, as_pil=False):
    """the `control_type == 'scribble'` branch of ControlNetHelper.prepare_conditioning_images (model/ctrl_helper.py:196-197:
    HEDdetector(img, scribble=True) per frame) for a whole clip -> uint8 [N, H, W, 3] on the GPU, or the list of PIL images.
    A PidiNetDetector gives PidiNetDetector(img, scribble=True) instead (the same tail behind PiDiNet's map)."""
    return _extract(frames, detector, True, as_pil)


def extract_softedge(frames, detector, as_pil=False):
    """the `control_type == 'softedge'` branch of ControlNetHelper.prepare_conditioning_images (model/ctrl_helper.py:184-185) for a whole
    clip -> uint8 [N, H, W, 3] on the GPU, or the list of PIL images.  The reference's soft-edge detector is PiDiNet: add_softedge_estimator
    (model/ctrl_helper.py:103-107) overwrites its HEDdetector with PidiNetDetector.from_pretrained('lllyasviel/Annotators'), so pass a
    ctrl_adapter_amd.PidiNetDetector for the map the released soft-edge adapters were trained on.  An HEDdetector gives HED's soft-edge
    map (HEDdetector(img), the condition of control_v11p_sd15_softedge), exactly as before."""
    return _extract(frames, detector, False, as_pil)
