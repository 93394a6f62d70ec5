"""The cases of the lineart tests (tests/test_gpu_lineart.py).  Map sizes are functions of the tiles and chunks that
ctrl_lineart_launch_shape reports, so the edges sit where the kernels have theirs whatever the tiles are."""
import torch

import lineart_ref as R

BATCHES = (1, 3)
IN_WIDTHS = (64, 128, 256)
CONVT_SIZES = ((1, 1), (3, 5), (16, 16))
CONVT_WIDTHS = ((256, 128), (128, 64))
DETECTOR_CASES = {"64x64": (1, 64, 64), "64x128": (1, 64, 128), "128x64": (1, 128, 64)}
PLAN_SIZES = ((64, 64), (64, 128))


def tile_sizes(th, tw):
    """8 x 8 and 12 x 20 (the reflection reaches across a whole tile), one tile exactly, a tile plus one row and one column, a tall and a
    wide strip of the narrowest legal map, 64 x 128 (many tiles)"""
    return [(8, 8), (12, 20), (th, tw), (th + 1, tw + 1), (5 * th + 3, 4), (4, 4 * tw + 5), (64, 128)]


def in_sizes(rows_per_block):
    """H x W of 1, of a few rows, of a non-multiple of every chunk (23 x 29 = 667 rows: ragged for 128, 256 and 512 rows per workgroup),
    of 4096 (whole chunks), and one row past a chunk of the widest maps"""
    return [(1, 1), (5, 7), (23, 29), (64, 64), (1, rows_per_block + 1)]


def valid_conv_cases():
    """M of 63 | 64 | 72 (the ring kernel's 64-row tile) and 255 | 256 | 272 (the wide tile's 256 rows), each as (N, H, W)"""
    return [(1, 7, 9), (1, 8, 8), (1, 9, 8), (1, 15, 17), (1, 16, 16), (1, 17, 16), (3, 5, 7)]


def stem_problem(N, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + H * 131 + W)
    fr = R.make_frames(seed + H + W, N, H, W)
    fr[..., 0] = fr[..., 0] // 3                     # red dark, blue bright: a swapped order moves every output
    fr[..., 2] = 255 - fr[..., 2] // 4
    fr[0, 0, 0] = torch.tensor([255, 0, 128], dtype=torch.uint8)
    fr[-1, -1, -1] = torch.tensor([0, 255, 7], dtype=torch.uint8)
    w = (torch.randn((64, 3, 7, 7), generator=g) * (4.0 / 147 ** 0.5)).float()
    return fr, w


def head_problem(N, H, W, seed=0):
    """x [N, 64, H, W] fp16 (the map BEFORE its reflection padding), w [1, 64, 7, 7], b [1]: logits of deviation about 2"""
    g = torch.Generator().manual_seed(seed + H * 131 + W)
    x = torch.randn((N, 64, H, W), generator=g).clamp_min(0).half()
    w = (torch.randn((1, 64, 7, 7), generator=g) * (2.0 / (3136 * 0.34) ** 0.5)).float()
    b = torch.tensor([0.3])
    return x, w, b


def in_problem(N, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + C + H * 131 + W)
    x = (torch.randn((N, C, H, W), generator=g) * 1.5 + 0.3 * torch.randn((N, C, 1, 1), generator=g)).half()
    res = torch.randn((N, C, H, W), generator=g).half()
    return x, res


def conv_problem(N, Ci, Co, H, W, seed=0, transposed=False):
    g = torch.Generator().manual_seed(seed + Ci + H * 131 + W)
    x = torch.randn((N, Ci, H, W), generator=g).half()
    shape = (Ci, Co, 3, 3) if transposed else (Co, Ci, 3, 3)
    w = (torch.randn(shape, generator=g) / (Ci * (2.25 if transposed else 9)) ** 0.5).half()
    return x, w
