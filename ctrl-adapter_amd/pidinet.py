"""PidiNetDetector -- controlnet_aux's PiDiNet annotator on libctrlhip: the detector the reference makes its `softedge` condition with.

`add_softedge_estimator` (model/ctrl_helper.py:103-107) builds an HEDdetector and overwrites it on the next line with
`PidiNetDetector.from_pretrained('lllyasviel/Annotators')`; `prepare_conditioning_images` (184-185) calls it once per frame.  Here a clip's
frames go to the GPU once: the stem, the fifteen fused pixel-difference blocks (depthwise 3x3 / 5x5 -> ReLU -> 1x1 on the matrix cores ->
skip, one launch each), the four dilated context heads, the side maps and the bilinear fuse are the kernels of csrc/pidinet.hip; with
scribble=True HED's tail kernels follow.  The uint8 maps stay on the device as [N, H, W, 3], slices of which `prepare_images` takes as they
are.  No CPU fallback.

Sizes: only inputs that controlnet_aux's `resize_image` would leave unchanged run -- H and W multiples of 64 and
min(H, W) == detect_resolution == image_resolution (the reference's 512 x 512 frames); anything else raises ValueError.  safe=True raises
NotImplementedError: the reference never sets it.

The input is 0..1 and the net has no normalisation layers; a forward in which an activation leaves the fp16 range raises RuntimeError
instead of returning a wrong map.  The real checkpoint's activation range is not known here (table5_pidinet.pth has not been run).
"""
import ctypes as C
import os

import torch

from . import _lib as L
from .hed import _as_u8_rgb

_WIDTHS = (60, 120, 240, 240)
_BLOCKS = (3, 4, 4, 4)
_DIL = 24


def pidinet_state_dict_spec():
    """(name, shape) of every parameter of controlnet_aux's pidinet() (PiDiNet(60, 'carv4', dil=24, sa=True)), `module.` stripped"""
    spec = [("init_block.weight", (_WIDTHS[0], 3, 3, 3))]
    cin = _WIDTHS[0]
    for s, (c, n) in enumerate(zip(_WIDTHS, _BLOCKS), 1):
        for j in range(1, n + 1):
            pre = "block%d_%d." % (s, j)
            spec.append((pre + "conv1.weight", (cin, 1, 3, 3)))
            spec.append((pre + "conv2.weight", (c, cin, 1, 1)))
            if s > 1 and j == 1:
                spec.append((pre + "shortcut.weight", (c, cin, 1, 1)))
                spec.append((pre + "shortcut.bias", (c,)))
            cin = c
    for i, c in enumerate(_WIDTHS):
        spec.append(("dilations.%d.conv1.weight" % i, (_DIL, c, 1, 1)))
        spec.append(("dilations.%d.conv1.bias" % i, (_DIL,)))
        for k in range(1, 5):
            spec.append(("dilations.%d.conv2_%d.weight" % (i, k), (_DIL, _DIL, 3, 3)))
        spec.append(("attentions.%d.conv1.weight" % i, (4, _DIL, 1, 1)))
        spec.append(("attentions.%d.conv1.bias" % i, (4,)))
        spec.append(("attentions.%d.conv2.weight" % i, (1, 4, 3, 3)))
        spec.append(("conv_reduces.%d.conv.weight" % i, (1, _DIL, 1, 1)))
        spec.append(("conv_reduces.%d.conv.bias" % i, (1,)))
    spec.append(("classifier.weight", (1, 4, 1, 1)))
    spec.append(("classifier.bias", (1,)))
    return spec


class PidiNetDetector:
    """controlnet_aux.PidiNetDetector over a libctrlhip plan.  `PidiNetDetector.from_state_dict(sd)` takes pidinet()'s state dict (with or
    without the checkpoint's `module.` prefix), `PidiNetDetector.from_pretrained(path)` a local table5_pidinet.pth (or the directory that
    holds it)."""

    def __init__(self, state_dict, device=None, ws_cap_bytes=0):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        device = torch.device(device) if device is not None else None
        if device is None or device.type != "cuda":
            raise RuntimeError("PidiNetDetector (libctrlhip) runs on the GPU only; there is no CPU fallback")
        self.device = device
        state_dict = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        self._params = {}
        for name, shape in pidinet_state_dict_spec():
            if name not in state_dict:
                raise KeyError("PidiNetDetector: the state dict has no %r (pidinet()'s keys are expected)" % name)
            v = state_dict[name]
            if tuple(v.shape) != tuple(shape):
                raise ValueError("PidiNetDetector: %r has shape %s, expected %s" % (name, tuple(v.shape), tuple(shape)))
            self._params[name] = v.detach().to(device=device, dtype=torch.float32).contiguous()
        self._cfg = L.PidiConfig(0, 0, int(ws_cap_bytes))
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
            L.check(L.lib().ctrl_pidi_create(C.byref(self._cfg), refs, len(self._params), L.cur_stream(), C.byref(h)))
        self._plan = h

    @classmethod
    def from_state_dict(cls, state_dict, **kw):
        return cls(state_dict, **kw)

    @classmethod
    def from_pretrained(cls, local_path, filename="table5_pidinet.pth", **kw):
        """loads a LOCAL checkpoint (a file, or a directory holding `filename`, also under annotator/ckpts); nothing is downloaded.  The
        checkpoint's `state_dict` entry is taken when it has one, and `module.` is stripped from its keys."""
        path = str(local_path)
        if os.path.isdir(path):
            tried = [os.path.join(path, filename), os.path.join(path, "annotator", "ckpts", filename)]
            path = next((p for p in tried if os.path.exists(p)), None)
            if path is None:
                raise FileNotFoundError("PidiNetDetector.from_pretrained: no %s under %s (local files only; nothing is downloaded)" % (filename, local_path))
        elif not os.path.exists(path):
            raise FileNotFoundError("PidiNetDetector.from_pretrained: %s does not exist (local files only; nothing is downloaded)" % path)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        return cls(ckpt["state_dict"] if "state_dict" in ckpt else ckpt, **kw)

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None:
                L.lib().ctrl_pidi_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    def to(self, device):
        """controlnet_aux's `.to("cuda")` (model/ctrl_helper.py:107): the plan already lives on its GPU; another device is refused"""
        d = torch.device(device)
        if d.type != self.device.type or (d.index is not None and d.index != self.device.index):
            raise ValueError("PidiNetDetector: the plan lives on %s; create another detector for %s" % (self.device, device))
        return self

    def workspace_bytes(self, N, H, W, scribble=False, frames_per_group=None):
        return int(L.lib().ctrl_pidi_ws_bytes(self._plan, int(N), int(H), int(W), int(bool(scribble)), int(frames_per_group or 0)))

    @torch.no_grad()
    def run(self, frames, scribble=False, apply_filter=False, channels=3, frames_per_group=None, return_logits=False):
        """frames uint8 [N, H, W, 3] (RGB) on the detector's GPU -> uint8 [N, H, W, 3] (channels=3) or [N, H, W]; with return_logits also the
        fp32 [N, H, W] output of the classifier in front of the sigmoid"""
        if channels not in (1, 3):
            raise ValueError("PidiNetDetector: channels must be 1 or 3")
        if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError("PidiNetDetector.run: frames must be a uint8 tensor [N, H, W, 3]")
        if frames.device != self.device:
            raise ValueError("PidiNetDetector.run: frames live on %s, the detector on %s" % (frames.device, self.device))
        fpg = 0 if frames_per_group is None else int(frames_per_group)
        if frames_per_group is not None and fpg < 1:
            raise ValueError("frames_per_group must be None or positive (got %r)" % (frames_per_group,))
        frames = frames.contiguous()
        N, H, W = frames.shape[:3]
        if N < 1 or H % 64 or W % 64 or H < 64 or W < 64:
            raise ValueError("PidiNetDetector: %d frames of %d x %d: at least one frame with H and W multiples of 64 is required (the sizes "
                             "controlnet_aux's resize_image produces)" % (N, H, W))
        out = torch.empty((N, H, W, 3) if channels == 3 else (N, H, W), dtype=torch.uint8, device=self.device)
        logits = torch.empty((N, H, W), dtype=torch.float32, device=self.device) if return_logits else None
        with torch.cuda.device(self.device):
            L.check(L.lib().ctrl_pidi_forward(self._plan, L.ptr(frames), N, H, W, int(bool(scribble)), int(bool(apply_filter)), channels,
                                              L.ptr(out), L.ptr(logits), fpg, L.cur_stream()))
        return (out, logits) if return_logits else out

    def __call__(self, input_image, detect_resolution=512, image_resolution=512, safe=False, scribble=False, apply_filter=False,
                 output_type="pil", frames_per_group=None):
        """controlnet_aux.PidiNetDetector.__call__ for one image or a list of frames of one size.  output_type "pil": a PIL image (a list
        for a list), "np": uint8 arrays, "pt": ONE uint8 tensor [N, H, W, 3] that stays on the GPU (what prepare_images takes)."""
        if safe:
            raise NotImplementedError("PidiNetDetector: safe=True (the quantised safe_step) is not implemented; the reference never sets it")
        if output_type not in ("pil", "np", "pt"):
            raise ValueError("PidiNetDetector: output_type must be 'pil', 'np' or 'pt'")
        single = not isinstance(input_image, (list, tuple)) and not (torch.is_tensor(input_image) and input_image.dim() == 4)
        images = [input_image] if single else list(input_image)
        try:
            frames = [_as_u8_rgb(i) for i in images]
        except ValueError as e:
            raise ValueError(str(e).replace("HEDdetector", "PidiNetDetector")) from None
        if not frames or any(f.shape != frames[0].shape for f in frames):
            raise ValueError("PidiNetDetector needs at least one image and all images of one size")
        H, W = frames[0].shape[:2]
        if H % 64 or W % 64 or min(H, W) != int(detect_resolution) or min(H, W) != int(image_resolution):
            raise ValueError("PidiNetDetector: a %d x %d image with detect_resolution=%s, image_resolution=%s would be resized by "
                             "controlnet_aux (INTER_AREA / LANCZOS4), which this library does not do: H and W must be multiples of 64 and "
                             "min(H, W) == detect_resolution == image_resolution" % (H, W, detect_resolution, image_resolution))
        src = torch.stack([f.to(self.device) for f in frames]).contiguous()
        out = self.run(src, scribble=scribble, apply_filter=apply_filter, channels=3, frames_per_group=frames_per_group)
        if output_type == "pt":
            return out
        host = out.cpu().numpy()
        if output_type == "pil":
            from PIL import Image
            res = [Image.fromarray(host[i]) for i in range(host.shape[0])]
        else:
            res = [host[i] for i in range(host.shape[0])]
        return res[0] if single else res
