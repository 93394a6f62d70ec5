"""canny / extract_canny -- the reference's canny condition extractor (model/ctrl_helper.py:171-179) on libctrlhip.

Per frame the reference runs `cv2.Canny(np.array(img), 100, 200)` on one host thread and stacks the edge map three times along the
channel axis (:177-178).  Here a clip's frames go to the GPU once and three HIP kernels (csrc/canny.hip) do OpenCV's arithmetic --
integer from the Sobel taps to the hysteresis, so the result is cv2's bit for bit -- for all frames together.  The edge maps come back
as uint8 device tensors, [N, H, W, 3] slices of which `prepare_images` takes as they are: from raw frame to the ControlNet's
`controlnet_cond` nothing returns to the host.  The hysteresis loop reads a flag back between passes, so a call synchronises its
stream and cannot be captured into a graph.  No CPU fallback.
"""
import ctypes as C
import math
import sys
import types

import numpy as np
import torch

from . import _lib as L

_ws = {}          # device -> the cached workspace (flag block + candidate map), grown on demand


def thresholds(low_threshold, high_threshold):
    """cv2.Canny's handling of its thresholds: swapped when low > high, then floored"""
    low, high = float(low_threshold), float(high_threshold)
    if math.isnan(low) or math.isnan(high):
        raise ValueError("canny: a threshold is NaN")
    if low > high:
        low, high = high, low
    return math.floor(low), math.floor(high)


def _as_u8(img):
    """-> uint8 tensor [H, W] or [H, W, 3] (host or device), as np.array(img) gives it for a PIL image"""
    if torch.is_tensor(img):
        a = img
        if a.dtype != torch.uint8 or a.dim() not in (2, 3) or (a.dim() == 3 and a.shape[2] != 3):
            raise ValueError("canny: tensor images must be uint8 [H, W, 3] or [H, W]")
        return a
    if hasattr(img, "convert"):                  # PIL image: np.array(img), as the reference does
        if getattr(img, "mode", None) not in ("RGB", "L"):
            raise ValueError("canny: PIL images must have mode RGB or L, not %r" % (getattr(img, "mode", None),))
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("canny: images must be PIL images (RGB or L) or uint8 [H, W, 3] / [H, W] arrays")
    return torch.from_numpy(np.array(a, copy=True, order="C"))


def _workspace(device, nbytes):
    key = str(device)
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


@torch.no_grad()
def canny(images, low_threshold=100, high_threshold=200, channels=1, device=None, return_stats=False):
    """cv2.Canny(image, low_threshold, high_threshold) of every image -> uint8 [N, H, W] (channels=1) or [N, H, W, 3] (the edge map
    three times, channels=3) on `device`.  `images`: PIL images (RGB or L), uint8 arrays or uint8 tensors, [H, W, 3] or [H, W], all of
    one size.  With return_stats also a dict(passes=, readbacks=) of the hysteresis loop."""
    if channels not in (1, 3):
        raise ValueError("canny: channels must be 1 or 3")
    low, high = thresholds(low_threshold, high_threshold)
    frames = [_as_u8(i) for i in images]
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("canny needs at least one image and all images of one size")
    if device is None:
        device = next((f.device for f in frames if f.is_cuda), None)
        device = device if device is not None else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
    device = torch.device(device) if device is not None else None
    if device is None or device.type != "cuda":
        raise RuntimeError("canny (libctrlhip) runs on the GPU only; there is no CPU fallback")
    src = torch.stack([f.to(device) for f in frames]).contiguous()          # [N][H][W] or [N][H][W][3] uint8
    N, H, W = src.shape[:3]
    Cin = 1 if src.dim() == 3 else 3
    lib = L.lib()
    out = torch.empty((N, H, W) if channels == 1 else (N, H, W, 3), dtype=torch.uint8, device=device)
    nbytes = int(lib.ctrl_canny_ws_bytes(N, H, W))
    if nbytes <= 0:
        raise ValueError("canny: %d images of %d x %d are more than one call handles (N*H*W*3 must stay below 2**31 bytes)" % (N, H, W))
    passes, readbacks = C.c_int(0), C.c_int(0)
    with torch.cuda.device(device):
        ws = _workspace(device, nbytes)
        L.check(lib.ctrl_canny(L.ptr(src), N, H, W, Cin, float(low), float(high), channels, L.ptr(out), L.ptr(ws), nbytes,
                               C.byref(passes), C.byref(readbacks), L.cur_stream()))
    if return_stats:
        return out, {"passes": passes.value, "readbacks": readbacks.value}
    return out


def extract_canny(images, as_pil=False):
    """the `control_type == 'canny'` branch of ControlNetHelper.prepare_conditioning_images: thresholds 100 / 200, the edge map on three
    channels.  -> uint8 [N, H, W, 3] on the GPU (its slices are what prepare_images takes), or with as_pil=True the list of PIL images
    the reference's pipelines expect."""
    out = canny(images, 100, 200, channels=3)
    if not as_pil:
        return out
    from PIL import Image
    host = out.cpu().numpy()
    return [Image.fromarray(host[i]) for i in range(host.shape[0])]


class _CallableModule(types.ModuleType):
    """The package exports the function `canny`, and this module has the same name: `import ctrl_adapter_amd.canny` rebinds the package's
    attribute to the module.  Calling the module calls the function, so `ctrl_adapter_amd.canny(...)` works either way."""

    def __call__(self, *args, **kwargs):
        return canny(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
