"""Restatement of controlnet_aux's PiDiNet annotator (pidinet() = PiDiNet(60, 'carv4', dil=24, sa=True) + PidiNetDetector.__call__), written
from knowledge of that package -- it is not installed here, so tests/test_pidinet_host.py pins this file to it wherever it exists
(importorskip).

  PiDiNetRef            the net as a plain torch module with controlnet_aux's state-dict keys (any dtype); every pixel-difference
                        convolution is computed ON THE FLY from its 3x3 weight, as controlnet_aux does
  convert_pdc           the vanilla 3x3 / 5x5 kernel that computes the same map (what the library's plan builds once)
  make_state_dict       seeded checkpoints: "he" (mixed sign, for the tests that compare the library with itself) and "calibrated"
                        (the whole-detector test: activations of order one in every block, side maps of unit deviation)
  forward               the detector up to its logits as a function of the state dict, fp64; emulate=True rounds to fp16 exactly where the
                        library stores or feeds fp16 (the stem's output, the depthwise result handed to the MFMA, every block's output, the
                        head's 24-channel map) and to fp32 where it keeps fp32 weights; the arithmetic stays fp64.  **planted: the errors the
                        checks must catch
  *_ref                 per-kernel fp64 references with element-wise bounds, built like helpers.igemm_bound:
                        (K + 8) 2^-24 sum|terms| for every fp32 sum of K terms in any order, 2^-11 |v| + 2^-25 for every fp16 store, the
                        depthwise stage's fp16 hand-over to the MFMA counted, every input error carried through |W|.  Nothing is measured.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIDTHS = (60, 120, 240, 240)
BLOCKS = (3, 4, 4, 4)
DIL = 24
DILATIONS = (5, 7, 9, 11)
KINDS = ("cd", "ad", "rd", "cv")                   # carv4: layer L (0 = init_block) has kind KINDS[L % 4]
KIND_CODE = {"cv": 0, "cd": 1, "ad": 2, "rd": 3}    # ctrl_pidi_convert_pdc
AD_FROM = [3, 0, 1, 6, 4, 2, 7, 8, 5]
RD_POS = [0, 2, 4, 10, 14, 20, 22, 24]
RD_NEG = [6, 7, 8, 11, 13, 16, 17, 18]
EPS = 2.0 ** -24
PLANTS = ("ad_inverted", "rd_first8", "cd_no_centre", "no_flip", "pool_after", "no_shortcut_bias", "wrong_dilation", "align_corners")


def layers():
    """(layer, stage 1..4, index 1.., kind, cin, cout, stride-2?) of the fifteen PDC blocks"""
    out, L, cin = [], 1, WIDTHS[0]
    for s, (c, n) in enumerate(zip(WIDTHS, BLOCKS), 1):
        for j in range(1, n + 1):
            out.append((L, s, j, KINDS[L % 4], cin, c, s > 1 and j == 1))
            cin = c
            L += 1
    return out


def spec():
    out = [("init_block.weight", (WIDTHS[0], 3, 3, 3))]
    for _, s, j, _, cin, c, pool in layers():
        pre = "block%d_%d." % (s, j)
        out.append((pre + "conv1.weight", (cin, 1, 3, 3)))
        out.append((pre + "conv2.weight", (c, cin, 1, 1)))
        if pool:
            out.append((pre + "shortcut.weight", (c, cin, 1, 1)))
            out.append((pre + "shortcut.bias", (c,)))
    for i, c in enumerate(WIDTHS):
        out.append(("dilations.%d.conv1.weight" % i, (DIL, c, 1, 1)))
        out.append(("dilations.%d.conv1.bias" % i, (DIL,)))
        for k in range(1, 5):
            out.append(("dilations.%d.conv2_%d.weight" % (i, k), (DIL, DIL, 3, 3)))
        out.append(("attentions.%d.conv1.weight" % i, (4, DIL, 1, 1)))
        out.append(("attentions.%d.conv1.bias" % i, (4,)))
        out.append(("attentions.%d.conv2.weight" % i, (1, 4, 3, 3)))
        out.append(("conv_reduces.%d.conv.weight" % i, (1, DIL, 1, 1)))
        out.append(("conv_reduces.%d.conv.bias" % i, (1,)))
    out.append(("classifier.weight", (1, 4, 1, 1)))
    out.append(("classifier.bias", (1,)))
    return out


# ------------------------------------------------------------------------------------------------------------- pixel-difference convs
def pdc_on_the_fly(kind, x, w, groups=1):
    """PiDiNet's ops.createConvFunc(kind) on a [Co, Ci / groups, 3, 3] weight, padding as the net uses it"""
    if kind == "cv":
        return F.conv2d(x, w, padding=1, groups=groups)
    if kind == "cd":
        y = F.conv2d(x, w, padding=1, groups=groups)
        return y - F.conv2d(x, w.sum(dim=(2, 3), keepdim=True), padding=0, groups=groups)
    f = w.reshape(w.shape[0], w.shape[1], 9)
    if kind == "ad":
        return F.conv2d(x, (f - f[:, :, AD_FROM]).reshape(w.shape), padding=1, groups=groups)
    assert kind == "rd", kind
    b = torch.zeros(w.shape[0], w.shape[1], 25, dtype=w.dtype, device=w.device)
    b[:, :, RD_POS] = f[:, :, 1:]
    b[:, :, RD_NEG] = -f[:, :, 1:]
    b[:, :, 12] = 0
    return F.conv2d(x, b.reshape(w.shape[0], w.shape[1], 5, 5), padding=2, groups=groups)


def convert_pdc(kind, w):
    """[Co, Ci, 3, 3] -> the vanilla kernel [Co, Ci, 3, 3] (cv, cd, ad) or [Co, Ci, 5, 5] (rd) in w's dtype"""
    f = w.reshape(w.shape[0], w.shape[1], 9)
    if kind == "cv":
        return w.clone()
    if kind == "cd":
        o = f.clone()
        o[:, :, 4] = f[:, :, 4] - f.sum(-1)
        return o.reshape(w.shape)
    if kind == "ad":
        return (f - f[:, :, AD_FROM]).reshape(w.shape)
    b = torch.zeros(w.shape[0], w.shape[1], 25, dtype=w.dtype, device=w.device)
    b[:, :, RD_POS] = f[:, :, 1:]
    b[:, :, RD_NEG] = -f[:, :, 1:]
    return b.reshape(w.shape[0], w.shape[1], 5, 5)


def _planted_kernel(kind, w, planted):
    """convert_pdc, or what a planted conversion error (ad permutation inverted, rd taking weights 0..7, cd without its centre) makes of w"""
    if not ({"ad_inverted", "rd_first8", "cd_no_centre"} & set(planted)):
        return convert_pdc(kind, w)
    f = w.reshape(w.shape[0], w.shape[1], 9)
    if kind == "cd" and "cd_no_centre" in planted:
        return w.clone()
    if kind == "ad" and "ad_inverted" in planted:
        return (f - f[:, :, [AD_FROM.index(i) for i in range(9)]]).reshape(w.shape)
    if kind == "rd" and "rd_first8" in planted:
        b = torch.zeros(w.shape[0], w.shape[1], 25, dtype=w.dtype, device=w.device)
        b[:, :, RD_POS] = f[:, :, :8]
        b[:, :, RD_NEG] = -f[:, :, :8]
        return b.reshape(w.shape[0], w.shape[1], 5, 5)
    return convert_pdc(kind, w)


# ------------------------------------------------------------------------------------------------------------- the module
class _PDC(torch.nn.Module):
    def __init__(self, kind, cin, cout, groups=1):
        super().__init__()
        self.kind, self.groups = kind, groups
        self.weight = torch.nn.Parameter(torch.zeros(cout, cin // groups, 3, 3))

    def forward(self, x):
        return pdc_on_the_fly(self.kind, x, self.weight, self.groups)


class _PDCBlock(torch.nn.Module):
    def __init__(self, kind, cin, cout, stride):
        super().__init__()
        self.stride = stride
        if stride > 1:
            self.shortcut = torch.nn.Conv2d(cin, cout, 1)
        self.conv1 = _PDC(kind, cin, cin, groups=cin)
        self.conv2 = torch.nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        if self.stride > 1:
            x = F.max_pool2d(x, 2, 2)
        y = self.conv2(F.relu(self.conv1(x)))
        if self.stride > 1:
            x = self.shortcut(x)
        return y + x


class _CDCM(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, cout, 1)
        for k, d in enumerate(DILATIONS, 1):
            setattr(self, "conv2_%d" % k, torch.nn.Conv2d(cout, cout, 3, dilation=d, padding=d, bias=False))

    def forward(self, x):
        x = self.conv1(F.relu(x))
        return self.conv2_1(x) + self.conv2_2(x) + self.conv2_3(x) + self.conv2_4(x)


class _CSAM(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(c, 4, 1)
        self.conv2 = torch.nn.Conv2d(4, 1, 3, padding=1, bias=False)

    def forward(self, x):
        return x * torch.sigmoid(self.conv2(self.conv1(F.relu(x))))


class _MapReduce(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(c, 1, 1)

    def forward(self, x):
        return self.conv(x)


class PiDiNetRef(torch.nn.Module):
    """controlnet_aux's pidinet(): x float BGR 0..1 NCHW -> the sigmoid of the four side maps and of the fused map"""

    def __init__(self):
        super().__init__()
        self.init_block = _PDC(KINDS[0], 3, WIDTHS[0])
        for _, s, j, kind, cin, c, pool in layers():
            setattr(self, "block%d_%d" % (s, j), _PDCBlock(kind, cin, c, 2 if pool else 1))
        self.dilations = torch.nn.ModuleList([_CDCM(c, DIL) for c in WIDTHS])
        self.attentions = torch.nn.ModuleList([_CSAM(DIL) for _ in WIDTHS])
        self.conv_reduces = torch.nn.ModuleList([_MapReduce(DIL) for _ in WIDTHS])
        self.classifier = torch.nn.Conv2d(4, 1, 1)

    def forward(self, x):
        H, W = x.shape[2:]
        x = self.init_block(x)
        es = []
        for s, n in enumerate(BLOCKS, 1):
            for j in range(1, n + 1):
                x = getattr(self, "block%d_%d" % (s, j))(x)
            e = self.conv_reduces[s - 1](self.attentions[s - 1](self.dilations[s - 1](x)))
            es.append(F.interpolate(e, (H, W), mode="bilinear", align_corners=False))
        out = self.classifier(torch.cat(es, dim=1))
        return [torch.sigmoid(r) for r in es + [out]]


def detector_u8(logit, apply_filter=False):
    """PidiNetDetector behind the net: sigmoid, optional > 0.5, (edge * 255).clip(0, 255).astype(uint8); logit float32 numpy"""
    edge = 1 / (1 + np.exp(-np.asarray(logit, dtype=np.float32)))
    if apply_filter:
        edge = (edge > 0.5).astype(np.float32)
    return (edge * 255.0).clip(0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- checkpoints and frames
def _f16(t):
    return t.half().float()


def make_frames(seed, N, H, W):
    """uint8 [N, H, W, 3]: smooth blobs plus noise, the three channels different"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((N, 3, H // 16, W // 16), generator=g)
    img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 200 + torch.rand((N, 3, H, W), generator=g) * 55
    return img.permute(0, 2, 3, 1).clamp(0, 255).to(torch.uint8).contiguous()


def takes_fp16(name):
    """the tensors the library feeds to the MFMA as fp16: every 1x1 of the blocks and the context heads' 1x1 and dilated convolutions"""
    if name.startswith("block"):
        return name.endswith("conv2.weight") or name.endswith("shortcut.weight")
    return name.startswith("dilations.") and name.endswith(".weight")


def make_state_dict(seed, kind="he", gain=1.0):
    """seeded fp32 state dict; the weights the library takes as fp16 are fp16-representable.
    "he": mixed-sign weights of deviation sqrt(1 / fan_in) (asymmetric 3x3 planes).  "calibrated": depthwise kernels whose converted form
    has unit L1, 1x1 rows non-negative with sum 0.6, shortcuts with normalised rows, a stem and heads scaled on a calibration frame so
    that the stem's output and every side map have unit deviation (side maps centred), a classifier that gives logits of deviation
    about 0.4.  gain multiplies the stem (the range-guard test)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in spec():
        if name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.2
        elif name == "classifier.weight":
            v = torch.tensor([0.3, -0.25, 0.2, 0.25]).reshape(shape) + torch.randn(shape, generator=g) * 0.02
        else:
            fan = shape[1] * shape[2] * shape[3]
            v = torch.randn(shape, generator=g) / math.sqrt(fan)
            if kind == "calibrated" and name.startswith("block") and name.endswith("conv2.weight"):
                v = torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) < 0.25)
                v = v / v.sum(dim=1, keepdim=True).clamp_min(1e-6) * 0.6
            if kind == "calibrated" and name.endswith("shortcut.weight"):
                v = v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1)
        sd[name] = v.float().contiguous()
    if kind == "calibrated":
        for L, s, j, k, cin, c, pool in layers():
            n = "block%d_%d.conv1.weight" % (s, j)
            l1 = convert_pdc(k, sd[n].double()).abs().flatten(1).sum(1).clamp_min(1e-6)
            sd[n] = (sd[n].double() / l1.reshape(-1, 1, 1, 1)).float()
    for name in sd:
        if takes_fp16(name):
            sd[name] = _f16(sd[name])
    if kind == "calibrated":
        _calibrate(sd)
    sd["init_block.weight"] = (sd["init_block.weight"] * gain).contiguous()
    return sd


def _calibrate(sd):
    cal = make_frames(99, 1, 64, 64)
    x = cal.permute(0, 3, 1, 2).double().flip(1) / 255.0
    y = pdc_on_the_fly("cd", x, sd["init_block.weight"].double())
    sd["init_block.weight"] = (sd["init_block.weight"] / float(y.std())).contiguous()
    st = _trunk(sd, cal, torch.float64, False, ())
    for i in range(4):
        s = _cdcm(sd, i, st[i], False, DILATIONS)
        raw = _side(sd, i, s, with_bias=False)
        k = float(raw.std().clamp_min(1e-9))
        sd["conv_reduces.%d.conv.weight" % i] = (sd["conv_reduces.%d.conv.weight" % i] / k).contiguous()
        sd["conv_reduces.%d.conv.bias" % i] = (-(raw.mean() / k)).reshape(1).float() + sd["conv_reduces.%d.conv.bias" % i] * 0.5
    es = [_side(sd, i, _cdcm(sd, i, st[i], False, DILATIONS)) for i in range(4)]
    up = torch.cat([F.interpolate(e, (64, 64), mode="bilinear", align_corners=False) for e in es], 1)
    lg = F.conv2d(up, sd["classifier.weight"].double())
    sd["classifier.bias"] = (-lg.mean()).reshape(1).float()


# ------------------------------------------------------------------------------------------------------------- the functional forward
def _trunk(sd, frames_u8, dtype, emulate, planted):
    """-> the four stage outputs [N, C, h, w]"""
    r16 = (lambda t: t.half().to(dtype)) if emulate else (lambda t: t)
    r32 = (lambda t: t.float().to(dtype)) if emulate else (lambda t: t)
    x = frames_u8.permute(0, 3, 1, 2)
    if "no_flip" not in planted:
        x = x.flip(1)
    x = (x.float() / 255.0).to(dtype) if emulate else x.to(dtype) / 255.0
    x = r16(F.conv2d(x, r32(_planted_kernel("cd", sd["init_block.weight"].to(dtype), planted)), padding=1))
    outs = []
    for L, s, j, kind, cin, c, pool in layers():
        pre = "block%d_%d." % (s, j)
        if pool and "pool_after" not in planted:
            x = F.max_pool2d(x, 2, 2)
        k = r32(_planted_kernel(kind, sd[pre + "conv1.weight"].to(dtype), planted))
        a = r16(F.relu(F.conv2d(x, k, padding=k.shape[-1] // 2, groups=cin)))
        y = F.conv2d(a, sd[pre + "conv2.weight"].to(dtype))
        if pool:
            y = y + F.conv2d(x, sd[pre + "shortcut.weight"].to(dtype), None if "no_shortcut_bias" in planted else sd[pre + "shortcut.bias"].to(dtype))
        else:
            y = y + x
        x = r16(y)
        if pool and "pool_after" in planted:
            x = F.max_pool2d(x, 2, 2)
        if j == BLOCKS[s - 1]:
            outs.append(x)
    return outs


def _cdcm(sd, i, x, emulate, dilations):
    dt = x.dtype
    pre = "dilations.%d." % i
    t = F.conv2d(F.relu(x), sd[pre + "conv1.weight"].to(dt), sd[pre + "conv1.bias"].to(dt))
    if emulate:
        t = t.half().to(dt)
    return sum(F.conv2d(t, sd[pre + "conv2_%d.weight" % (k + 1)].to(dt), padding=d, dilation=d) for k, d in enumerate(dilations))


def _side(sd, i, s, with_bias=True):
    dt = s.dtype
    a = F.conv2d(F.relu(s), sd["attentions.%d.conv1.weight" % i].to(dt), sd["attentions.%d.conv1.bias" % i].to(dt))
    y = torch.sigmoid(F.conv2d(a, sd["attentions.%d.conv2.weight" % i].to(dt), padding=1))
    return F.conv2d(s * y, sd["conv_reduces.%d.conv.weight" % i].to(dt), sd["conv_reduces.%d.conv.bias" % i].to(dt) if with_bias else None)


def forward(sd, frames_u8, dtype=torch.float64, emulate=False, **planted):
    """the detector's logits [N, H, W] (the classifier's output in front of the sigmoid).  planted: any of PLANTS = True"""
    bad = set(planted) - set(PLANTS)
    assert not bad, bad
    planted = tuple(k for k, v in planted.items() if v)
    N, H, W = frames_u8.shape[:3]
    st = _trunk(sd, frames_u8, dtype, emulate, planted)
    dil = DILATIONS if "wrong_dilation" not in planted else (5, 7, 7, 11)
    es = [_side(sd, i, _cdcm(sd, i, st[i], emulate, dil)) for i in range(4)]
    up = torch.cat([F.interpolate(e, (H, W), mode="bilinear", align_corners="align_corners" in planted) for e in es], 1)
    return F.conv2d(up, sd["classifier.weight"].to(dtype), sd["classifier.bias"].to(dtype))[:, 0]


def detector_tolerance(sd, frames_u8):
    """(fp64 logits, tolerance): 4 x max |emulated - fp64| over the same frames.  The factor 4 covers fp16 ties that the fp32 summation
    order flips the other way and their propagation; the fp32 sums themselves sit three orders below the fp16 stores."""
    ref = forward(sd, frames_u8)
    emu = forward(sd, frames_u8, emulate=True)
    dev = float((emu - ref).abs().max())
    return ref, emu, dev, 4.0 * dev


def outside(got, ref, tol):
    """number of pixels with |got - ref| > tol (every pixel is compared)"""
    got, ref = torch.as_tensor(np.asarray(got), dtype=torch.float64), torch.as_tensor(np.asarray(ref), dtype=torch.float64)
    return int((~((got - ref).abs() <= tol)).sum())


# ------------------------------------------------------------------------------------------------------------- packing for the op entries
def cp(c):
    return (c + 63) // 64 * 64


def pack_stem(kernel):
    """converted init kernel [60, 3, 3, 3] (net channel order) -> fp32 [9][3][64]"""
    o = torch.zeros(9, 3, 64)
    o[:, :, :kernel.shape[0]] = kernel.float().reshape(kernel.shape[0], 3, 9).permute(2, 1, 0)
    return o.contiguous()


def pack_dw(kernel):
    """converted depthwise kernel [C, 1, k, k] -> fp32 [k * k][CP]"""
    C, taps = kernel.shape[0], kernel.shape[-1] ** 2
    o = torch.zeros(taps, cp(C))
    o[:, :C] = kernel.float().reshape(C, taps).t()
    return o.contiguous()


def pack_1x1(w, rows_p=None):
    """[Co, Ci, 1, 1] -> fp16 [rows_p or CP(Co)][CP(Ci)], zero padded"""
    Co, Ci = w.shape[:2]
    o = torch.zeros(rows_p or cp(Co), cp(Ci), dtype=torch.float16)
    o[:Co, :Ci] = w.reshape(Co, Ci).half()
    return o.contiguous()


def pack_vec(b, n):
    o = torch.zeros(n)
    o[:b.numel()] = b.float().reshape(-1)
    return o.contiguous()


def pack_dilated(ws):
    """four [24, 24, 3, 3] -> fp16 [36][32][32]: [dilation][ky][kx] x cout x cin"""
    o = torch.zeros(36, 32, 32, dtype=torch.float16)
    for k, w in enumerate(ws):
        o[k * 9:(k + 1) * 9, :DIL, :DIL] = w.half().reshape(DIL, DIL, 9).permute(2, 0, 1)
    return o.contiguous()


def head_par(sd, i):
    """(par124, par37) of head i as float lists: att [4][24] | att_b [4] | red [24];  side w [ky][kx][4] | red bias"""
    p = torch.cat([sd["attentions.%d.conv1.weight" % i].reshape(-1), sd["attentions.%d.conv1.bias" % i].reshape(-1),
                   sd["conv_reduces.%d.conv.weight" % i].reshape(-1)]).float()
    q = torch.cat([sd["attentions.%d.conv2.weight" % i].reshape(4, 9).t().reshape(-1), sd["conv_reduces.%d.conv.bias" % i].reshape(-1)]).float()
    return [float(v) for v in p], [float(v) for v in q]


def pad_nhwc(x_nchw, dtype=torch.float16):
    """[N, C, H, W] -> NHWC with the channels zero padded to CP(C)"""
    N, C, H, W = x_nchw.shape
    o = torch.zeros(N, H, W, cp(C), dtype=dtype)
    o[..., :C] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return o


# ------------------------------------------------------------------------------------------------------------- per-kernel references
def _store16(ref, err):
    """bound after one fp16 round-to-nearest of a value known to err"""
    return err + 2.0 ** -11 * (ref.abs() + err) + 2.0 ** -25


def stem_ref(frames_u8, kernel):
    """kernel: the converted [60, 3, 3, 3] (fp32 values).  -> (ref, bound) [N, 60, H, W]; 27 taps, one more rounding per term for x / 255"""
    x = frames_u8.permute(0, 3, 1, 2).double().flip(1) / 255.0
    k = kernel.double()
    ref = F.conv2d(x, k, padding=1)
    mag = F.conv2d(x, k.abs(), padding=1)
    return ref, _store16(ref, (28 + 8) * EPS * mag)


def block_ref(x16, dwk, w2, wsc=None, bsc=None, pool=False):
    """x16 [N, C, H, W] fp16 values; dwk the converted depthwise kernel [C, 1, k, k] (fp32 values); w2 / wsc fp16 values [Co, C, 1, 1].
    -> (ref, bound) [N, Co, Ho, Wo]"""
    x = x16.double()
    if pool:
        x = F.max_pool2d(x, 2, 2)
    C = x.shape[1]
    k = dwk.double()
    taps = k.shape[-1] ** 2
    pre = F.conv2d(x, k, padding=k.shape[-1] // 2, groups=C)
    e1 = (taps + 8) * EPS * F.conv2d(x.abs(), k.abs(), padding=k.shape[-1] // 2, groups=C)
    a = F.relu(pre)
    ea = _store16(a, e1)                            # the fp16 hand-over to the MFMA
    W2 = w2.double()
    ref = F.conv2d(a, W2)
    mag = F.conv2d(a + ea, W2.abs())
    err = F.conv2d(ea, W2.abs())
    K = C
    if wsc is not None:
        ref = ref + F.conv2d(x, wsc.double(), bsc.double())
        mag = mag + F.conv2d(x.abs(), wsc.double().abs(), bsc.double().abs())
        K = 2 * C + 1
    else:
        ref = ref + x
        mag = mag + x.abs()
        K = C + 1
    err = err + (K + 8) * EPS * mag
    return ref, _store16(ref, err)


def head_reduce_ref(x16, w1, b1):
    """-> (ref, bound) [N, 24, H, W] of t = w1 . relu(x) + b1 stored as fp16"""
    a = F.relu(x16.double())
    ref = F.conv2d(a, w1.double(), b1.double())
    mag = F.conv2d(a, w1.double().abs(), b1.double().abs())
    return ref, _store16(ref, (x16.shape[1] + 1 + 8) * EPS * mag)


def head_context_ref(t16, ws, att_w, att_b, red_w):
    """t16 [N, 24, H, W] fp16 values, ws the four dilated weights.  -> (a4, a4 bound, d, d bound); a4 [N, 4, H, W], d [N, 1, H, W]"""
    t = t16.double()
    s = sum(F.conv2d(t, w.double(), padding=dl, dilation=dl) for w, dl in zip(ws, DILATIONS))
    smag = sum(F.conv2d(t.abs(), w.double().abs(), padding=dl, dilation=dl) for w, dl in zip(ws, DILATIONS))
    es = (36 * DIL + 8) * EPS * smag
    A, b, r = att_w.double(), att_b.double(), red_w.double()
    a4 = F.conv2d(F.relu(s), A, b)
    a4b = F.conv2d(es, A.abs()) + (DIL + 1 + 8) * EPS * F.conv2d(F.relu(s) + es, A.abs(), b.abs())
    d = F.conv2d(s, r)
    db = F.conv2d(es, r.abs()) + (DIL + 8) * EPS * F.conv2d(s.abs() + es, r.abs())
    return a4, a4b, d, db


def side_ref(a4, d, w, b):
    """a4 [N, 4, H, W], d [N, 1, H, W] fp32 values (exact inputs), w [1, 4, 3, 3], b [1] -> (e, bound) [N, 1, H, W]"""
    a4, d, w = a4.double(), d.double(), w.double()
    z = F.conv2d(a4, w, padding=1)
    ez = (36 + 8) * EPS * F.conv2d(a4.abs(), w.abs(), padding=1)
    sg = torch.sigmoid(z)
    esg = ez / 4 + 2.0 ** -21 * sg                  # |sigmoid'| <= 1/4; expf, the sum and the division: a few ulp
    ref = sg * d + b.double()
    return ref, esg * d.abs() + 4 * EPS * ((sg * d).abs() + b.double().abs())


def fuse_ref(es, cw, cb, H, W):
    """es: four [N, h, w] fp32 maps (exact inputs), cw [4], cb scalar -> (logit, bound) [N, H, W].  The bilinear weights are exact
    (dyadic); about three roundings per pass and the four-term sum: 16 ulp of the magnitude"""
    ref = torch.zeros(es[0].shape[0], H, W, dtype=torch.float64) + float(cb)
    mag = torch.zeros_like(ref) + abs(float(cb))
    for e, w in zip(es, cw):
        up = F.interpolate(e.double()[:, None], (H, W), mode="bilinear", align_corners=False)[:, 0]
        upa = F.interpolate(e.double().abs()[:, None], (H, W), mode="bilinear", align_corners=False)[:, 0]
        ref = ref + float(w) * up
        mag = mag + abs(float(w)) * upa
    return ref, 16 * EPS * mag
