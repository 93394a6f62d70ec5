"""The cases of the PiDiNet tests (tests/test_pidinet_host.py, tests/test_gpu_pidinet.py).  Map sizes are functions of the tiles that
ctrl_pidi_launch_shape reports, so the edges sit where the kernels have theirs whatever the tiles are."""
import ctypes as C

import numpy as np
import torch

import pidinet_ref as R

KINDS = ("cd", "ad", "rd", "cv")
IDENTITY_WIDTHS = ((60, 60), (120, 120), (240, 240))
POOL_WIDTHS = ((60, 120), (120, 240), (240, 240))
BATCHES = (1, 3)
HEAD_WIDTHS = (60, 120, 240)
FUSE_SIZES = ((64, 64), (64, 128), (128, 64))          # (128, 64): a tall map
DETECTOR_CASES = {"64x64": (1, 64, 64), "64x128": (2, 64, 128), "128x64": (2, 128, 64)}
PAD_GARBAGE = 777.0                     # finite; what an input's pad channels hold in the second run of a block form


def block_forms():
    """(kind, cin, cout, pool): four kinds (two tap footprints) x three widths x {identity, pool + shortcut}"""
    return [(k, ci, co, pool) for k in KINDS for pool, widths in ((False, IDENTITY_WIDTHS), (True, POOL_WIDTHS)) for ci, co in widths]


def block_sizes(th, tw):
    """OUTPUT map sizes (the pooled forms read a map twice as large): 8 x 8 -- smaller than a tile; rd's 2-pixel halo meets all four
    borders at once --, exactly one tile, a tile plus one row and one column"""
    return [(8, 8), (th, tw), (th + 1, tw + 1)]


def head_sizes(ts):
    """8 x 8 (every non-centre tap of dilations 9 and 11 falls outside), 16 x 24, a tile plus one each way"""
    return [(8, 8), (16, 24), (ts + 1, ts + 1)]


def block_problem(kind, cin, cout, pool, N, Ho, Wo, seed):
    """operands of one block form as fp32 / fp16-valued CPU tensors: x [N, cin, H, W], the 3x3 depthwise weight, w2, wsc, bsc"""
    g = torch.Generator().manual_seed(seed)
    H, W = (2 * Ho, 2 * Wo) if pool else (Ho, Wo)
    x = (torch.randn((N, cin, H, W), generator=g) * 1.5).half()
    w1 = (torch.randn((cin, 1, 3, 3), generator=g) / 3 + 0.05 * torch.arange(9.0).reshape(1, 1, 3, 3)).float()     # asymmetric planes
    w2 = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).half()
    wsc = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).half() if pool else None
    bsc = torch.randn(cout, generator=g).float() if pool else None
    return x, w1, w2, wsc, bsc


def head_problem(C, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((N, C, H, W), generator=g) * 1.5).half()
    w1 = (torch.randn((R.DIL, C, 1, 1), generator=g) / C ** 0.5).half()
    b1 = (torch.randn(R.DIL, generator=g) * 0.3).float()
    ws = [(torch.randn((R.DIL, R.DIL, 3, 3), generator=g) / (R.DIL * 9 * 4) ** 0.5 * 2).half() for _ in range(4)]
    att_w = (torch.randn((4, R.DIL, 1, 1), generator=g) / R.DIL ** 0.5).float()
    att_b = (torch.randn(4, generator=g) * 0.3).float()
    red_w = (torch.randn((1, R.DIL, 1, 1), generator=g) / R.DIL ** 0.5).float()
    side_w = (torch.randn((1, 4, 3, 3), generator=g) / 3).float()
    red_b = (torch.randn(1, generator=g) * 0.3).float()
    return x, w1, b1, ws, att_w, att_b, red_w, side_w, red_b


def lib_convert(kind, w):
    """ctrl_pidi_convert_pdc on a CPU fp32 tensor [Co, Ci, 3, 3] -> fp32 [Co, Ci, k, k]"""
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    co, ci = w.shape[:2]
    k = 5 if kind == "rd" else 3
    src = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    out = np.empty((co, ci, k, k), np.float32)
    fp = C.POINTER(C.c_float)
    rc = lib.ctrl_pidi_convert_pdc(R.KIND_CODE[kind], src.ctypes.data_as(fp), co, ci, out.ctypes.data_as(fp))
    assert rc == 0, lib.ctrl_last_error().decode()
    return torch.from_numpy(out)
