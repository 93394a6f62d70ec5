"""Restatement of controlnet_aux's HED annotator (ControlNetHED_Apache2 + HEDdetector.__call__), written from knowledge of that package
and of OpenCV -- neither is installed here, so tests/test_hed_host.py pins this file to them wherever they exist (importorskip).

  ControlNetHEDRef      the net as a plain torch module with controlnet_aux's state-dict keys (any dtype)
  logits_and_bound      the same forward in fp64 together with a running element-wise bound of what an fp16-activation / fp32-accumulation
                        implementation may differ by (derivation below)
  resize_linear / fuse  cv2.resize(INTER_LINEAR) as cv2 computes it, and the mean / sigmoid / uint8 step
  gaussian_taps / blur / nms / scribble_tail   the scribble post-processing in ONE fixed arithmetic order (numpy float32): rows before
                        columns, taps from left to right, every tap one rounded multiply and one rounded add -- csrc/hed.hip follows it bit for bit

The bound.  Every activation carries (v, e): the fp64 value and a bound of |computed - v|.
  conv + ReLU  e_out = |W| * e_in                                   the input's error through the linear map
                     + (K + 8) 2^-24 (|W| * (|v_in| + e_in) + |b|)   a length-K fp32 sum in any order (tests/helpers.py: igemm_bound)
                     + |W - fp16(W)| * (|v_in| + e_in)               the weights as the MFMA takes them (0 for the test checkpoints)
               ReLU is 1-Lipschitz; the stored fp16 adds 2^-11 (|v_out| + e_out) + 2^-25 / s   (s: the trunk scale; the subnormal step is
               taken in the scaled units)
  max-pool     e_out = max-pool(e_in)    (|max a - max b| <= max |a - b|)
  projection   e_p = |w| . e + (C + 8) 2^-24 (|w| . (|v| + e) + |b|)
  fuse         the bilinear weights are exact (dyadic); three roundings per pass, five terms and one division:
               e_l = mean_k R(e_k) + 16 * 2^-24 * mean_k R(|p_k| + e_k),   R = the resize
  uint8        floor(255 sigma(l - e_l) (1 - 2^-20)) <= out <= floor(255 sigma(l + e_l) (1 + 2^-20)): expf, the division and two products in
               fp32 are good to a few ulp; 2^-20 = 16 ulp
Worst-case propagation through |W| is only useful when |W| * |v| stays near |W * v|: the checkpoint kind "bounded" (make_state_dict) has a
non-negative, sparse trunk for that reason.  With mixed-sign He weights the bound grows by about 0.6 sqrt(K) per layer and says nothing after
thirteen layers; those checkpoints serve the tests that compare the library with itself or with the exact tail.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (64, 128, 256, 512, 512)
LAYERS = (2, 2, 3, 3, 3)


def spec():
    out = [("norm", (1, 3, 1, 1))]
    cin = 3
    for k, (c, n) in enumerate(zip(CHANNELS, LAYERS), 1):
        for j in range(n):
            out.append(("block%d.convs.%d.weight" % (k, j), (c, cin, 3, 3)))
            out.append(("block%d.convs.%d.bias" % (k, j), (c,)))
            cin = c
        out.append(("block%d.projection.weight" % k, (1, c, 1, 1)))
        out.append(("block%d.projection.bias" % k, (1,)))
    return out


def _f16(t):
    return t.half().float()


def make_state_dict(seed, kind="he", act_gain=1.0):
    """seeded fp32 state dict whose conv weights are fp16-representable.
    kind "he": He-initialised mixed-sign weights (std sqrt(2 / fan_in)), the stem divided by 64 for the 0..255 input, so that the logits
    spread over the sigmoid.  kind "bounded": a non-negative sparse trunk (about 4 taps per output channel, calibrated to activations near 1,
    negative biases so that ReLU clamps) under a signed stem, with non-negative sparse projections centred by their biases -- the checkpoints the derived bound is useful for.
    act_gain multiplies the stem's weights and bias (the range-guard test drives block 1 out of the fp16 range with it)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in spec():
        if name == "norm":
            v = torch.tensor([104.25, 116.5, 122.75]).reshape(1, 3, 1, 1) + torch.randn(shape, generator=g)
        elif name.endswith("projection.weight"):
            v = torch.randn(shape, generator=g) * (1.5 / math.sqrt(shape[1]))
            if kind == "bounded":       # no cancellation in the side output either: the bias centres it
                v = v.abs() * (torch.rand(shape, generator=g) < 0.25)
        elif name.endswith("projection.bias"):
            v = torch.randn(shape, generator=g) * 0.5
        elif name == "block1.convs.0.weight":
            v = _f16(torch.randn(shape, generator=g) * math.sqrt(2.0 / 27) / (64 if kind == "he" else 16) * act_gain)
        elif name == "block1.convs.0.bias":
            v = torch.randn(shape, generator=g) * 0.5 * act_gain
        elif name.endswith(".weight"):
            K = shape[1] * 9
            if kind == "he":
                v = _f16(torch.randn(shape, generator=g) * math.sqrt(2.0 / K))
            else:
                keep = torch.rand(shape, generator=g) < 4.0 / K
                v = torch.rand(shape, generator=g) * keep
        else:
            v = torch.randn(shape, generator=g) * (0.05 if kind == "he" else 0.3) - (0.0 if kind == "he" else 0.4)
        sd[name] = v.float().contiguous()
    if kind == "bounded":
        _calibrate(sd)
    return sd


def _calibrate(sd):
    """the bounded checkpoint keeps its activations near 1 through all thirteen layers: every trunk conv is scaled so that its output
    has mean 1 on a fixed calibration frame before the (negative) bias, every projection so that its map has mean 0 and deviation 1"""
    v = make_frames(99, 1, 64, 64).permute(0, 3, 1, 2).float() - sd["norm"]
    for k in range(5):
        if k:
            v = F.max_pool2d(v, 2, 2)
        for j in range(LAYERS[k]):
            wn, bn = "block%d.convs.%d.weight" % (k + 1, j), "block%d.convs.%d.bias" % (k + 1, j)
            if k + j:
                raw = F.conv2d(v, sd[wn], None, padding=1)
                sd[wn] = _f16(sd[wn] / raw.mean().clamp_min(1e-6))
            v = F.relu(F.conv2d(v, sd[wn], sd[bn], padding=1))
        wn, bn = "block%d.projection.weight" % (k + 1), "block%d.projection.bias" % (k + 1)
        p = F.conv2d(v, sd[wn], None)
        sd[wn] = (sd[wn] / p.std().clamp_min(1e-6)).contiguous()
        sd[bn] = -F.conv2d(v, sd[wn], None).mean().reshape(1) + sd[bn] * 0.2


def make_frames(seed, N, H, W):
    """uint8 [N, H, W, 3]: smooth blobs plus noise, so that edges exist at every scale"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((N, 3, H // 16, W // 16), generator=g)
    img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 200 + torch.rand((N, 3, H, W), generator=g) * 55
    return img.permute(0, 2, 3, 1).clamp(0, 255).to(torch.uint8).contiguous()


class _Block(torch.nn.Module):
    def __init__(self, cin, cout, layers):
        super().__init__()
        self.convs = torch.nn.Sequential(*[torch.nn.Conv2d(cin if j == 0 else cout, cout, 3, padding=1) for j in range(layers)])
        self.projection = torch.nn.Conv2d(cout, 1, 1)

    def forward(self, x, down_sampling=False):
        h = F.max_pool2d(x, 2, 2) if down_sampling else x
        for conv in self.convs:
            h = F.relu(conv(h))
        return h, self.projection(h)


class ControlNetHEDRef(torch.nn.Module):
    """controlnet_aux's ControlNetHED_Apache2: x float RGB 0..255 NCHW -> the five projection maps at strides 1, 2, 4, 8, 16"""

    def __init__(self):
        super().__init__()
        self.norm = torch.nn.Parameter(torch.zeros(1, 3, 1, 1))
        cin = 3
        for k, (c, n) in enumerate(zip(CHANNELS, LAYERS), 1):
            setattr(self, "block%d" % k, _Block(cin, c, n))
            cin = c

    def forward(self, x):
        h = x - self.norm
        outs = []
        for k in range(1, 6):
            h, p = getattr(self, "block%d" % k)(h, down_sampling=k > 1)
            outs.append(p)
        return tuple(outs)


def logits_and_bound(sd, frames_u8, trunk_scale=1.0, pool_blocks=(1, 2, 3, 4), no_relu_last=None, align_corners=False, want_bound=True):
    """fp64 forward of the detector up to the mean logit [N, H, W], with the running bound of the module docstring.
    Planted errors: pool_blocks (0-based blocks that begin with the max-pool), no_relu_last (0-based block whose last conv has no ReLU),
    align_corners (the fuse)."""
    x = frames_u8.permute(0, 3, 1, 2).double() - sd["norm"].double()
    v, e = x, x.abs() * 2.0 ** -24
    N, _, H, W = x.shape
    maps = []
    for k in range(5):
        if k in pool_blocks:
            v, e = F.max_pool2d(v, 2, 2), F.max_pool2d(e, 2, 2)
        for j in range(LAYERS[k]):
            w = sd["block%d.convs.%d.weight" % (k + 1, j)].double()
            b = sd["block%d.convs.%d.bias" % (k + 1, j)].double()
            K = w.shape[1] * 9
            out = F.conv2d(v, w, b, padding=1)
            if want_bound:
                a = v.abs() + e
                mag = F.conv2d(a, w.abs(), b.abs(), padding=1)
                err = F.conv2d(e, w.abs(), None, padding=1) + (K + 8) * 2.0 ** -24 * mag
                wr = (w - w.float().half().double()).abs()
                if k + j > 0 and float(wr.max()) > 0:
                    err = err + F.conv2d(a, wr, None, padding=1)
            if not (no_relu_last == k and j == LAYERS[k] - 1):
                out = out.clamp_min(0)
            v = out
            if want_bound:
                e = err + 2.0 ** -11 * (v.abs() + err) + 2.0 ** -25 / trunk_scale
        pw = sd["block%d.projection.weight" % (k + 1)].double()
        pb = sd["block%d.projection.bias" % (k + 1)].double()
        p = F.conv2d(v, pw, pb)
        pe = None
        if want_bound:
            pe = F.conv2d(e, pw.abs()) + (pw.shape[1] + 8) * 2.0 ** -24 * F.conv2d(v.abs() + e, pw.abs(), pb.abs())
        maps.append((p[:, 0], pe[:, 0] if want_bound else None))
    acc = torch.zeros((N, H, W), dtype=torch.float64)
    E = torch.zeros_like(acc)
    A = torch.zeros_like(acc)
    for p, pe in maps:
        for n in range(N):
            acc[n] += torch.from_numpy(resize_linear(p[n].numpy(), H, W, align_corners))
            if want_bound:
                E[n] += torch.from_numpy(resize_linear(pe[n].numpy(), H, W, align_corners))
                A[n] += torch.from_numpy(resize_linear(p[n].abs().numpy(), H, W, align_corners))
    logit = acc / 5
    bound = E / 5 + 16 * 2.0 ** -24 * (A + E) / 5 if want_bound else None
    return logit, bound


# ------------------------------------------------------------------------------------------------------------- the fuse
def _lin_coords(dst, src, align_corners):
    """cv2.resize INTER_LINEAR: fx = (dx + 0.5) * scale - 0.5 in float, floor, clamped at both borders"""
    d = np.arange(dst, dtype=np.float64)
    if align_corners:
        f = d * ((src - 1) / max(dst - 1, 1))
    else:
        f = (d + 0.5) * (src / dst) - 0.5
    f = f.astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo = s < 0
    s[lo], f[lo] = 0, 0
    hi = s >= src - 1
    s[hi], f[hi] = src - 1, 0
    return s, np.minimum(s + 1, src - 1), f.astype(np.float32)


def resize_linear(e, H, W, align_corners=False):
    """cv2.resize(e, (W, H), interpolation=cv2.INTER_LINEAR) of a 2-D map, in the map's dtype (float32 as cv2; float64 for the bound);
    the row pass first, then the column pass; an equal size is a copy"""
    if e.shape == (H, W):
        return e.copy()
    dt = e.dtype.type
    x0, x1, fx = _lin_coords(W, e.shape[1], align_corners)
    y0, y1, fy = _lin_coords(H, e.shape[0], align_corners)
    fx, fy = fx.astype(e.dtype), fy.astype(e.dtype)
    rows = e[:, x0] * (dt(1) - fx) + e[:, x1] * fx
    return rows[y0] * (dt(1) - fy)[:, None] + rows[y1] * fy[:, None]


def fuse(maps, H, W, align_corners=False):
    """HEDdetector: the five maps (float32 2-D) resized, edge = 1 / (1 + exp(-mean)), (edge * 255).clip(0, 255).astype(uint8).
    -> (uint8 [H, W], the float32 mean)"""
    edges = [resize_linear(np.asarray(m, dtype=np.float32), H, W, align_corners) for m in maps]
    mean = np.mean(np.stack(edges, axis=2), axis=2)
    edge = 1 / (1 + np.exp(-mean.astype(np.float32)))
    return (edge * 255.0).clip(0, 255).astype(np.uint8), mean


def u8_interval(logit, bound):
    """the uint8 values the module docstring's bound allows per pixel (fp64 in, int64 lo / hi out)"""
    logit, bound = np.asarray(logit, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    lo = np.floor(255.0 * sig(logit - bound) * (1 - 2.0 ** -20)).clip(0, 255).astype(np.int64)
    hi = np.floor(255.0 * sig(logit + bound) * (1 + 2.0 ** -20)).clip(0, 255).astype(np.int64)
    return lo, hi


# ------------------------------------------------------------------------------------------------------------- the checks
def logit_failures(got, ref, bound):
    """number of pixels whose logit lies outside ref +- bound"""
    got, ref, bound = (np.asarray(t, dtype=np.float64) for t in (got, ref, bound))
    return int((~(np.abs(got - ref) <= bound)).sum())


def u8_failures(got_u8, ref_logit, bound):
    lo, hi = u8_interval(ref_logit, bound)
    g = np.asarray(got_u8).astype(np.int64)
    return int(((g < lo) | (g > hi)).sum())


def exact_failures(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got != want).sum())


# ------------------------------------------------------------------------------------------------------------- the scribble tail
def gaussian_taps(n, sigma=3.0):
    """cv2.getGaussianKernel(n, sigma) for a float kernel: exp in double, normalised in double, cast to float (libm's exp and a
    left-to-right sum, exactly as csrc/hed.hip computes its table)"""
    e = [math.exp(-((i - (n - 1) * 0.5) ** 2) / (2.0 * sigma * sigma)) for i in range(n)]
    s = 0.0
    for v in e:
        s += v
    return np.array([v / s for v in e], dtype=np.float64).astype(np.float32)


def auto_ksize(sigma, is_u8):
    """cv2.GaussianBlur with ksize (0, 0): round(sigma * (3 if uint8 else 4) * 2 + 1) | 1"""
    return int(round(sigma * (3 if is_u8 else 4) * 2 + 1)) | 1


def _pad(x, r, border):
    return np.pad(x, r, mode="reflect" if border == "reflect101" else "symmetric")


def blur(x, taps, border="reflect101"):
    """separable blur of a 2-D float32 map in the fixed order: the row pass (taps left to right), then the column pass (top to bottom)"""
    assert x.dtype == np.float32 and taps.dtype == np.float32
    n = len(taps)
    r = n // 2
    H, W = x.shape
    p = _pad(x, r, border)
    acc = p[:, 0:W] * taps[0]
    for t in range(1, n):
        acc = acc + p[:, t:t + W] * taps[t]
    acc2 = acc[0:H] * taps[0]
    for t in range(1, n):
        acc2 = acc2 + acc[t:t + H] * taps[t]
    assert acc2.dtype == np.float32
    return acc2


def nms(x_u8, t=127, s=3.0, directions=4, ksize=None, border="reflect101"):
    """controlnet_aux.util.nms: blur the float32 map, keep a pixel where cv2.dilate(x, f) == x for one of the four 3-pixel line kernels
    (neighbours outside the image do not count), 255 where the kept value is > t"""
    x = blur(x_u8.astype(np.float32), gaussian_taps(ksize or auto_ksize(s, False), s), border)
    return nms_keep(x, t, directions), x


def nms_keep(x, t=127, directions=4):
    """the part of nms behind its blur, on a float32 map"""
    H, W = x.shape
    p = np.pad(x, 1, mode="constant", constant_values=-np.inf)
    c = p[1:H + 1, 1:W + 1]
    lines = [((1, 0), (1, 2)), ((0, 1), (2, 1)), ((0, 0), (2, 2)), ((0, 2), (2, 0))][:directions]
    keep = np.zeros((H, W), dtype=bool)
    for (ay, ax), (by, bx) in lines:
        d = np.maximum(np.maximum(p[ay:ay + H, ax:ax + W], p[by:by + H, bx:bx + W]), c)
        keep |= d == c
    y = np.where(keep, x, np.float32(0))
    return np.where(y > t, 255, 0).astype(np.uint8)


def blur_u8_bin(z_u8, s=3.0, ksize=None, border="reflect101"):
    """cv2.GaussianBlur(z, (0, 0), s) on uint8 (rounded half to even, saturated), then map[map > 4] = 255; map[map < 255] = 0"""
    b = blur(z_u8.astype(np.float32), gaussian_taps(ksize or auto_ksize(s, True), s), border)
    u = np.rint(b).clip(0, 255).astype(np.uint8)
    return np.where(u > 4, 255, 0).astype(np.uint8)


def scribble_tail(soft_u8, **planted):
    """HEDdetector(scribble=True) behind the soft map: nms(map, 127, 3.0), GaussianBlur(sigma 3), binarise.  planted: directions,
    border, swap_ksize"""
    k1 = k2 = None
    if planted.get("swap_ksize"):
        k1, k2 = auto_ksize(3.0, True), auto_ksize(3.0, False)
    border = planted.get("border", "reflect101")
    z, _ = nms(soft_u8, 127, 3.0, planted.get("directions", 4), k1, border)
    return blur_u8_bin(z, 3.0, k2, border)


def tail_maps(H, W, seed=0):
    """synthetic uint8 maps for the tail kernels: isolated pixels at corners and borders (the reflect-101), one-pixel lines in the four
    directions, plateaus (dilate == x ties), a random map"""
    rng = np.random.RandomState(seed)
    maps = {}
    m = np.zeros((H, W), np.uint8)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 3), (H // 3, W - 1), (1, 1), (H - 2, W - 2)):
        m[y, x] = 255
    maps["isolated"] = m
    m = np.zeros((H, W), np.uint8)
    m[H // 4, :] = 255
    m[:, W // 4] = 230
    for i in range(min(H, W)):
        m[i, i] = 210
        m[i, W - 1 - i] = 190
    maps["lines"] = m
    m = np.zeros((H, W), np.uint8)
    m[4:20, 6:30] = 200
    m[H - 12:, W - 24:] = 255
    m[H // 2:H // 2 + 9, :] = 140
    maps["plateaus"] = m
    maps["random"] = (rng.rand(H, W) ** 0.5 * 255).astype(np.uint8)
    soft = np.zeros((H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    soft = 128 + 120 * np.sin(xx / 5.0) * np.cos(yy / 7.0)
    maps["waves"] = soft.clip(0, 255).astype(np.uint8)
    return maps
