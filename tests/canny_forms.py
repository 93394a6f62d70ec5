"""The cases of the canny tests (tests/test_canny_host.py, tests/test_gpu_canny.py): the golden pairs, the sizes, thresholds and input
images of the map kernel, and the synthetic candidate maps of the hysteresis.  Everything is a function of the tile (th, tw) that
ctrl_canny_launch_shape reports, so the edges sit where the kernels have theirs whatever the tile is."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canny")
# (input, cv2.Canny(input, 100, 200) on three channels as the reference's authors stored it): tests/golden/canny/README.md
PAIRS = [("frames/raw_input/camel/00000.png", "frames/canny/camel/00000.png"),
         ("frames/raw_input/newspaper_cat/00000.png", "frames/canny/newspaper_cat/00000.png"),
         ("images/raw_input/crown_frog_512.png", "images/canny/crown_frog.png")]
_cache = {}


def load_pair(i):
    """(input uint8 [512, 512, 3], cv2's output uint8 [512, 512, 3]) of golden pair i, read once and never changed"""
    if i not in _cache:
        from PIL import Image
        a, b = (np.array(Image.open(os.path.join(GOLD, p))) for p in PAIRS[i])
        assert a.dtype == np.uint8 and a.shape == (512, 512, 3) and b.dtype == np.uint8 and b.shape == (512, 512, 3)
        assert np.array_equal(b[..., 0], b[..., 1]) and np.array_equal(b[..., 0], b[..., 2])      # ctrl_helper.py:177-178
        assert set(np.unique(b)) <= {0, 255}
        a.setflags(write=False)
        b.setflags(write=False)
        _cache[i] = (a, b)
    return _cache[i]


# ---- map kernel ---------------------------------------------------------------------------------------------------------------
THRESHOLDS = [(100, 200), (0, 0), (200, 100), (2040, 3000), (99.9, 200.5)]


def map_sizes(th, tw):
    """(H, W): the degenerate sizes, every size one short of / at / one past the tile in both axes, and two sizes of several ragged tiles"""
    return [(1, 1), (1, 7), (5, 1), (2, 2), (3, 3)] + [(h, w) for h in (th - 1, th, th + 1) for w in (tw - 1, tw, tw + 1)] + [(33, 65), (97, 130)]


def _box_blur(a, k):
    p = np.pad(a.astype(np.float64), ((k, k), (k, k), (0, 0)), mode="edge")
    out = np.zeros(a.shape, np.float64)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out += p[dy:dy + a.shape[0], dx:dx + a.shape[1]]
    return out / (2 * k + 1) ** 2


def blurred_noise(H, W, C, seed):
    """box-blurred noise stretched back to the full range: gradients from nothing to well past 200, so a map of it holds none, weak and
    strong pixels (tests assert that wherever the size allows it)"""
    g = np.random.default_rng(seed)
    b = _box_blur(g.integers(0, 256, size=(H, W, C)), 1)
    b = (b - b.min()) / max(b.max() - b.min(), 1.0)
    return np.clip(np.rint(b * 255.0), 0, 255).astype(np.uint8)


def map_inputs(H, W, C, seed):
    """name -> uint8 [H, W, C]"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    rep = lambda a: np.repeat(a[:, :, None], C, axis=2).astype(np.uint8)
    lohi = lambda mask, lo=30, hi=200: np.where(mask, hi, lo)
    out = {
        "noise": g.integers(0, 256, size=(H, W, C), dtype=np.uint8),
        "blurred": blurred_noise(H, W, C, seed + 1),
        # step edges: a step between two flat halves gives a ridge two pixels wide with EQUAL magnitudes: only the > / >= asymmetry picks one
        "step_h": rep(lohi(yy >= H // 2)),
        "step_v": rep(lohi(xx >= W // 2)),
        "step_d1": rep(lohi(xx + yy >= (H + W) // 2)),
        "step_d2": rep(lohi(xx - yy >= (W - H) // 2)),
        # the same steps at an amplitude whose magnitude lies between the thresholds 100 and 200 of most cases (weak everywhere)
        "step_weak": rep(lohi((xx >= W // 2) ^ (yy >= H // 2), 100, 140)),
        # edges on the outermost rows and columns: a bright one-pixel frame, and a dark one
        "frame": rep(lohi((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1), 10, 250)),
        "frame_inv": rep(lohi((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1), 250, 10)),
    }
    if C == 3:
        # three channels whose magnitudes tie at EVERY pixel with different signs: A(x) + B(y), its negative, and B(y) - A(x) (the Sobel
        # pair is linear: dx negated, dy kept).  Where the two steps cross, the gradient is diagonal and channel 2 points along the
        # other diagonal than channels 0 and 1: only the first-max rule says which neighbours are compared.
        A, B = np.where(xx >= W // 2, 60, 0), np.where(yy >= H // 2, 60, 0)
        tie = np.stack([30 + A + B, 225 - A - B, 90 - A + B], axis=2).astype(np.uint8)
        out["tie"] = tie
        out["tie_rev"] = np.ascontiguousarray(tie[:, :, ::-1])
    return out


# ---- hysteresis ---------------------------------------------------------------------------------------------------------------
def serpentine(H, W, step=8):
    """a one-pixel path of weak pixels: full-width rows every `step` rows, joined at alternating ends, one strong pixel at its far end.
    (crossings() counts its tile-edge crossings)"""
    m = np.zeros((H, W), np.uint8)
    rows = list(range(0, H, step))
    for k, r in enumerate(rows):
        m[r, :] = 1
        if k + 1 < len(rows):
            c = W - 1 if k % 2 == 0 else 0
            m[r:rows[k + 1] + 1, c] = 1
    # row k runs left to right when k is even: the path ends at the far end of the last row
    m[rows[-1], W - 1 if (len(rows) - 1) % 2 == 0 else 0] = 2
    return m


def crossings(m, th, tw):
    """how often the non-zero pixels of a one-pixel path step over a tile edge: horizontally or vertically adjacent pairs that straddle one"""
    nz = m != 0
    h = nz[:, :-1] & nz[:, 1:]
    v = nz[:-1, :] & nz[1:, :]
    cols = np.arange(1, m.shape[1]) % tw == 0
    rows = np.arange(1, m.shape[0]) % th == 0
    return int(h[:, cols].sum() + v[rows, :].sum())


def hysteresis_maps(th, tw, seed=3):
    """name -> candidate map uint8 (values 0, 1, 2); all but "ragged*" are 3 th x 3 tw"""
    H, W = 3 * th, 3 * tw
    g = np.random.default_rng(seed)
    out = {"serpentine": serpentine(H, W)}
    # chains that cross the point where four tiles meet by diagonal steps only: (th, tw) down the main diagonal, (th, 2 tw) down the other
    m = np.zeros((H, W), np.uint8)
    for k in range(-6, 7):
        m[th + k, tw + k] = 1
        m[th + k, 2 * tw - 1 - k] = 1
    m[th - 6, tw - 6] = 2                          # strong in the upper-left tile: promotes through the corner into the lower-right one
    m[th + 6, 2 * tw - 7] = 2                      # strong in the lower-left of that junction: promotes up and to the right
    out["diagonal_junctions"] = m
    # weak components with no strong pixel stay: blobs that straddle tile edges, a strong pixel that touches none of them
    m = np.zeros((H, W), np.uint8)
    m[th - 3:th + 3, tw - 3:tw + 3] = 1
    m[2 * th - 1:2 * th + 1, 5:W - 5] = 1
    m[5, 5] = 2
    out["weak_only_components"] = m
    out["all_none"] = np.zeros((H, W), np.uint8)
    out["all_weak"] = np.ones((H, W), np.uint8)
    out["all_strong"] = np.full((H, W), 2, np.uint8)
    # a strong pixel in each corner of the map, each with a weak arm along the border and one into the interior
    m = np.zeros((H, W), np.uint8)
    m[0, :tw + 2] = 1; m[:th + 2, W - 1] = 1; m[H - 1, W - tw - 2:] = 1; m[H - th - 2:, 0] = 1
    for k in range(1, 9):
        m[k, k] = 1; m[k, W - 1 - k] = 1; m[H - 1 - k, k] = 1; m[H - 1 - k, W - 1 - k] = 1
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 2
    out["corners"] = m
    # random maps: many weak pixels, few strong ones, so components are large, winding and partly unreachable
    out["random"] = g.choice(np.array([0, 1, 2], np.uint8), size=(H, W), p=[0.52, 0.47, 0.01])
    out["ragged"] = g.choice(np.array([0, 1, 2], np.uint8), size=(2 * th + 1, 2 * tw - 1), p=[0.52, 0.47, 0.01])
    out["ragged_serpentine"] = serpentine(2 * th + 1, 2 * tw - 1, step=6)
    return out
