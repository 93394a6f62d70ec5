"""OpenCV's Canny (apertureSize 3, L2gradient False) restated in numpy, the reference of the canny tests.

    canny(img, low, high)         uint8 [H, W] or [H, W, C] -> uint8 [H, W] of 0 / 255: cv2.Canny(img, low, high)
    candidate_map(img, low, high) the intermediate the map kernel writes: 0 no candidate, 1 weak, 2 strong
    hysteresis(map)               flood fill: every 1 that is 8-connected to a 2 through non-zero pixels becomes 2

tests/test_canny_host.py pins it to cv2's own outputs (tests/golden/canny/).  `plant` names ONE deliberate error (PLANTS); the host test
checks that every one of them but the tangent constant moves pixels on every golden, i.e. that the goldens can tell.

The arithmetic: per channel the 3x3 Sobel pair over a replicated border, in int; per pixel the FIRST channel with the largest |dx| + |dy|
gives dx, dy and the magnitude m; m outside the image is 0.  A pixel is a candidate when m > low and m is a maximum along its gradient's
direction class -- horizontal (|dy| << 15 < |dx| * TG22): m > left and m >= right; vertical (|dy| << 15 > |dx| * TG22 + (|dx| << 16)): m > up
and m >= down; diagonal: m > both neighbours on the diagonal the signs of dx and dy pick.  TG22 = 13573 = (int)(tan(22.5 deg) * 2**15 + 0.5)
is OpenCV's source's constant: the goldens do not tell it from 13572.  Thresholds: swapped when low > high, then floored.
"""
import math

import numpy as np

TG22 = 13573
PLANTS = ("left_ge", "right_gt", "diag_ge", "conn4", "last_max_channel", "low_ge", "high_ge", "reflect_border", "flip_diagonal",
          "l2_magnitude", "tangent_13572")


def thresholds(low, high):
    """cv2's handling: swap when low > high, then floor"""
    if low > high:
        low, high = high, low
    return int(math.floor(low)), int(math.floor(high))


def gradients(img, plant=None):
    """-> dx, dy, m (int64 [H, W]) of the chosen channel"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    if a.ndim == 2:
        a = a[:, :, None]
    p = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect" if plant == "reflect_border" and min(a.shape[:2]) > 1 else "edge")
    H, W = a.shape[:2]

    def s(dr, dc):
        return p[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    n = np.abs(dx) + np.abs(dy)
    if plant == "last_max_channel":
        k = n.shape[2] - 1 - np.argmax(n[:, :, ::-1], axis=2)
    else:
        k = np.argmax(n, axis=2)                      # the first maximal channel
    take = lambda v: np.take_along_axis(v, k[:, :, None], axis=2)[:, :, 0]
    dx, dy = take(dx), take(dy)
    if plant == "l2_magnitude":
        m = np.floor(np.sqrt((dx * dx + dy * dy).astype(np.float64))).astype(np.int64)
    else:
        m = np.abs(dx) + np.abs(dy)
    return dx, dy, m


def candidate_map(img, low=100, high=200, plant=None):
    low, high = thresholds(low, high)
    dx, dy, m = gradients(img, plant)
    H, W = m.shape
    mp = np.pad(m, 1)                                 # the magnitude is 0 outside the image

    def nb(dr, dc):
        return mp[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * (13572 if plant == "tangent_13572" else TG22)
    t67 = t22 + (x << 16)
    gt, ge = np.greater, np.greater_equal
    horiz = (gt if plant != "left_ge" else ge)(m, nb(0, -1)) & (ge if plant != "right_gt" else gt)(m, nb(0, 1))
    vert = gt(m, nb(-1, 0)) & ge(m, nb(1, 0))
    neg = (dx ^ dy) < 0
    if plant == "flip_diagonal":
        neg = ~neg
    dcmp = gt if plant != "diag_ge" else ge
    diag = np.where(neg, dcmp(m, nb(-1, 1)) & dcmp(m, nb(1, -1)), dcmp(m, nb(-1, -1)) & dcmp(m, nb(1, 1)))
    cand = np.where(y < t22, horiz, np.where(y > t67, vert, diag))
    cand &= (m >= low) if plant == "low_ge" else (m > low)
    strong = (m >= high) if plant == "high_ge" else (m > high)
    return np.where(cand, np.where(strong, 2, 1), 0).astype(np.uint8)


def hysteresis(cmap, plant=None):
    """plain flood fill from the strong pixels over the non-zero ones"""
    out = np.array(cmap, dtype=np.uint8, copy=True)
    H, W = out.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if plant != "conn4":
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    stack = [(int(r), int(c)) for r, c in zip(*np.nonzero(out == 2))]
    while stack:
        r, c = stack.pop()
        for dr, dc in steps:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and out[rr, cc] == 1:
                out[rr, cc] = 2
                stack.append((rr, cc))
    return out


def canny(img, low=100, high=200, plant=None):
    assert plant is None or plant in PLANTS
    return np.where(hysteresis(candidate_map(img, low, high, plant), plant) == 2, 255, 0).astype(np.uint8)
