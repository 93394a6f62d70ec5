"""Restatement of controlnet_aux's lineart annotator (LineartDetector over two Generator(3, 1, 3) nets), written from knowledge of that
package -- it is not installed here, so tests/test_lineart_host.py pins this file to torch's own layers and, wherever controlnet_aux exists,
to the package itself (importorskip).

  GeneratorRef          the net from torch's own layers with controlnet_aux's state-dict keys: ReflectionPad2d, Conv2d, InstanceNorm2d
                        (no affine parameters, no running statistics, eps 1e-5, biased variance), ConvTranspose2d, Sigmoid
  forward               the detector up to its logits (model4.1's output in front of the sigmoid) as a function of the state dict, fp64;
                        emulate=True follows the library's arithmetic: the biases in front of an InstanceNorm dropped, every convolution's
                        output rounded to fp16, the statistics taken in fp32 as sum and sum of squares of those fp16 values
                        (var = max(sumsq / HW - mean^2, 0)), the normalised value + ReLU + residual in fp32 and rounded to fp16 once; the
                        sums of the convolutions themselves stay fp64.  **planted: the errors the checks must catch
  detector_u8           the byte rule behind the net: 255 - uint8(clip(255 sigmoid(logit))) by truncation
  make_state_dict       seeded checkpoints, N(0, 1 / fan_in) per layer -- with an InstanceNorm behind every convolution but the last, the
                        scale of those layers does not matter.  "calibrated": model4.1 is scaled and shifted on a calibration frame so that
                        the logits have a deviation of about 2 (the map takes far more than 20 levels)
  *_ref                 per-kernel fp64 references with element-wise bounds, built like helpers.igemm_bound: (K + 8) 2^-24 sum|terms| for
                        every fp32 sum of K terms in any order, 2^-11 |v| + 2^-25 for every fp16 store.  Nothing is measured.

Frames are random textures, never constant: on a constant frame every channel of the stem has zero variance and InstanceNorm normalises
rounding noise to unit variance.  controlnet_aux does exactly that too, so such an input has no meaningful answer, here or there.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
IN_EPS = 1e-5
PLANTS = ("bgr", "zero_pad", "unbiased_var", "convT_as_cout_cin")
CONV_KEYS = ["model1.0", "model1.3"] + ["model2.%d.conv_block.%d" % (b, j) for b in range(3) for j in (1, 5)]
CONVT_KEYS = ["model3.0", "model3.3"]


def spec():
    out = []

    def both(name, shape, cout):
        out.append((name + ".weight", shape))
        out.append((name + ".bias", (cout,)))

    both("model0.1", (64, 3, 7, 7), 64)
    both("model1.0", (128, 64, 3, 3), 128)
    both("model1.3", (256, 128, 3, 3), 256)
    for b in range(3):
        for j in (1, 5):
            both("model2.%d.conv_block.%d" % (b, j), (256, 256, 3, 3), 256)
    both("model3.0", (256, 128, 3, 3), 128)
    both("model3.3", (128, 64, 3, 3), 64)
    both("model4.1", (1, 64, 7, 7), 1)
    return out


# ------------------------------------------------------------------------------------------------------------- the module
class _ResidualBlock(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        nn = torch.nn
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c), nn.ReLU(inplace=True),
                                        nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c))

    def forward(self, x):
        return x + self.conv_block(x)


class GeneratorRef(torch.nn.Module):
    """controlnet_aux's lineart Generator(input_nc=3, output_nc=1, n_residual_blocks=3, sigmoid=True): x float RGB 0..1 NCHW -> [N, 1, H, W]"""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.model0 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(3, 64, 7), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        self.model1 = nn.Sequential(nn.Conv2d(64, 128, 3, stride=2, padding=1), nn.InstanceNorm2d(128), nn.ReLU(inplace=True),
                                    nn.Conv2d(128, 256, 3, stride=2, padding=1), nn.InstanceNorm2d(256), nn.ReLU(inplace=True))
        self.model2 = nn.Sequential(*[_ResidualBlock(256) for _ in range(3)])
        self.model3 = nn.Sequential(nn.ConvTranspose2d(256, 128, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(128),
                                    nn.ReLU(inplace=True),
                                    nn.ConvTranspose2d(128, 64, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(64),
                                    nn.ReLU(inplace=True))
        self.model4 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(64, 1, 7), nn.Sigmoid())

    def forward(self, x):
        return self.model4(self.model3(self.model2(self.model1(self.model0(x)))))

    def logits(self, x):
        """the value in front of the sigmoid"""
        x = self.model3(self.model2(self.model1(self.model0(x))))
        return self.model4[1](self.model4[0](x))


def detector_u8(logit, rounding=False, inverted=True):
    """LineartDetector behind the net: (sigmoid * 255).clip(0, 255).astype(uint8), then 255 - map; logit float32 numpy.
    rounding / inverted=False: the planted byte rules"""
    line = 1 / (1 + np.exp(-np.asarray(logit, dtype=np.float32)))
    v = (line * 255.0).clip(0, 255)
    m = (np.rint(v) if rounding else v).astype(np.uint8)
    return (255 - m) if inverted else m


# ------------------------------------------------------------------------------------------------------------- checkpoints and frames
def _f16(t):
    return t.half().float()


def make_frames(seed, N, H, W):
    """uint8 [N, H, W, 3]: smooth blobs plus noise, the three channels different, never constant"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((N, 3, max(2, H // 16), max(2, W // 16)), generator=g)
    img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 200 + torch.rand((N, 3, H, W), generator=g) * 55
    return img.permute(0, 2, 3, 1).clamp(0, 255).to(torch.uint8).contiguous()


def takes_fp16(name):
    """the tensors the library feeds to the MFMA as fp16: every 3x3 convolution and both transposed ones"""
    return name.endswith(".weight") and name[:-7] in CONV_KEYS + CONVT_KEYS


def make_state_dict(seed, kind="calibrated", gain=1.0, bias_seed=None):
    """seeded fp32 state dict; the weights the library takes as fp16 are fp16-representable.  Weights N(0, 1 / fan_in), biases N(0, 0.2^2)
    (those in front of an InstanceNorm drawn from bias_seed when given: two dicts that differ in the dropped biases only); "calibrated": model4.1 scaled and shifted so that the
    logits of a calibration frame have mean 0 and deviation 2.  gain multiplies the stem's weight (the range-guard test)."""
    assert kind in ("plain", "calibrated"), kind
    g = torch.Generator().manual_seed(seed)
    gb = torch.Generator().manual_seed(bias_seed) if bias_seed is not None else None
    sd = {}
    for name, shape in spec():
        if name.endswith(".bias"):
            v = torch.randn(shape, generator=g) * 0.2
            if gb is not None and name != "model4.1.bias":
                v = torch.randn(shape, generator=gb) * 0.2
        else:
            fan = (shape[0] if name[:-7] in CONVT_KEYS else shape[1]) * shape[2] * shape[3]
            v = torch.randn(shape, generator=g) / math.sqrt(fan)
        sd[name] = (_f16(v) if takes_fp16(name) else v.float()).contiguous()
    if kind == "calibrated":
        cal = make_frames(99, 1, 64, 64)
        raw = forward({n: (torch.zeros_like(v) if n.endswith(".bias") else v) for n, v in sd.items()}, cal)      # (whatever the biases)
        k = 2.0 / float(raw.std().clamp_min(1e-9))
        sd["model4.1.weight"] = (sd["model4.1.weight"] * k).contiguous()
        sd["model4.1.bias"] = (-(raw.mean() * k)).reshape(1).float()
    sd["model0.1.weight"] = (sd["model0.1.weight"] * gain).contiguous()
    return sd


# ------------------------------------------------------------------------------------------------------------- the functional forward
def reflect_pad(x, p):
    return F.pad(x, (p, p, p, p), mode="reflect")


def _inorm(t, emulate, unbiased, relu, res=None):
    """InstanceNorm2d (+ ReLU, + residual) of a convolution's output t.  emulate: t rounded to fp16, fp32 statistics from sum and sum of
    squares, fp32 arithmetic, one fp16 rounding of the result"""
    dt = t.dtype
    if not emulate:
        mean = t.mean(dim=(2, 3), keepdim=True)
        var = t.var(dim=(2, 3), keepdim=True, unbiased=unbiased)
        y = (t - mean) / torch.sqrt(var + IN_EPS)
        if relu:
            y = F.relu(y)
        return y if res is None else res + y
    x = t.half().float()
    hw = float(x.shape[2] * x.shape[3])
    inv = torch.tensor(1.0 / hw, dtype=torch.float32)
    mean = x.sum(dim=(2, 3), keepdim=True) * inv
    var = ((x * x).sum(dim=(2, 3), keepdim=True) * inv - mean * mean).clamp_min(0)
    if unbiased:
        var = var * (hw / (hw - 1))
    y = (x - mean) * torch.rsqrt(var + torch.tensor(IN_EPS, dtype=torch.float32))
    if relu:
        y = F.relu(y)
    if res is not None:
        y = y + res.float()
    return y.half().to(dt)


def forward(sd, frames_u8, dtype=torch.float64, emulate=False, **planted):
    """the detector's logits [N, H, W] (model4.1's output in front of the sigmoid).  planted: any of PLANTS = True"""
    bad = set(planted) - set(PLANTS)
    assert not bad, bad
    planted = {k for k, v in planted.items() if v}
    pad = (lambda x, p: F.pad(x, (p, p, p, p))) if "zero_pad" in planted else reflect_pad
    ub = "unbiased_var" in planted
    W_ = lambda n: sd[n + ".weight"].to(dtype)
    B_ = lambda n: None if emulate else sd[n + ".bias"].to(dtype)       # the library drops every bias in front of an InstanceNorm
    x = frames_u8.permute(0, 3, 1, 2)
    if "bgr" in planted:
        x = x.flip(1)
    x = (x.float() / 255.0).to(dtype) if emulate else x.to(dtype) / 255.0
    w0 = sd["model0.1.weight"].float().to(dtype) if emulate else W_("model0.1")
    x = _inorm(F.conv2d(pad(x, 3), w0, B_("model0.1")), emulate, ub, True)
    x = _inorm(F.conv2d(x, W_("model1.0"), B_("model1.0"), stride=2, padding=1), emulate, ub, True)
    x = _inorm(F.conv2d(x, W_("model1.3"), B_("model1.3"), stride=2, padding=1), emulate, ub, True)
    for b in range(3):
        k1, k2 = "model2.%d.conv_block.1" % b, "model2.%d.conv_block.5" % b
        y = _inorm(F.conv2d(pad(x, 1), W_(k1), B_(k1)), emulate, ub, True)
        x = _inorm(F.conv2d(pad(y, 1), W_(k2), B_(k2)), emulate, ub, False, res=x)
    for k in CONVT_KEYS:
        w = W_(k)
        if "convT_as_cout_cin" in planted:
            w = w.reshape(w.shape[1], w.shape[0], 3, 3).permute(1, 0, 2, 3)
        x = _inorm(F.conv_transpose2d(x, w, B_(k), stride=2, padding=1, output_padding=1), emulate, ub, True)
    return F.conv2d(pad(x, 3), W_("model4.1"), sd["model4.1.bias"].to(dtype))[:, 0]


def detector_tolerance(sd, frames_u8):
    """(fp64 logits, emulated logits, deviation, tolerance): 4 x max |emulated - fp64| over the same frames.  The factor 4 is the project's
    own (tests/test_gpu_pidinet.py): it covers fp16 ties that the fp32 summation order flips the other way and their propagation; the
    fp32 sums themselves sit three orders below the fp16 stores."""
    ref = forward(sd, frames_u8)
    emu = forward(sd, frames_u8, emulate=True)
    dev = float((emu - ref).abs().max())
    return ref, emu, dev, 4.0 * dev


def outside(got, ref, tol):
    """number of pixels with |got - ref| > tol (every pixel is compared)"""
    got, ref = torch.as_tensor(np.asarray(got), dtype=torch.float64), torch.as_tensor(np.asarray(ref), dtype=torch.float64)
    return int((~((got - ref).abs() <= tol)).sum())


def u8_interval(logit, bound):
    """the bytes 255 - floor(255 sigmoid(z)) a logit within `bound` of `logit` may give (int64 lo / hi)"""
    logit, bound = np.asarray(logit, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    m_lo = np.floor(255.0 * sig(logit - bound) * (1 - 2.0 ** -20)).clip(0, 255).astype(np.int64)
    m_hi = np.floor(255.0 * sig(logit + bound) * (1 + 2.0 ** -20)).clip(0, 255).astype(np.int64)
    return 255 - m_hi, 255 - m_lo


def u8_failures(got_u8, ref_logit, bound):
    """bytes that are the byte of NO logit inside the bound; every element is compared"""
    lo, hi = u8_interval(ref_logit, bound)
    g = np.asarray(got_u8).astype(np.int64)
    return int(((g < lo) | (g > hi)).sum())


# ------------------------------------------------------------------------------------------------------------- packing for the op entries
def pack_stem(w):
    """[64, 3, 7, 7] -> fp32 [49][3][64]"""
    return w.float().reshape(64, 3, 49).permute(2, 1, 0).contiguous()


def pack_head(w):
    """[1, 64, 7, 7] -> fp32 [49][64]"""
    return w.float().reshape(64, 49).t().contiguous()


def pack_conv(w):
    """[Co, Ci, 3, 3] -> fp16 [Co][9][Ci]"""
    return w.half().permute(0, 2, 3, 1).reshape(w.shape[0], 9 * w.shape[1]).contiguous()


def pack_convT_phase(w, planted=False):
    """ConvTranspose2d weight [Ci, Co, 3, 3] -> fp16 [4][Co][4][Ci]: phase 2a + b, tap 2ty + tx takes w[ci][co][ky][kx] with
    (a, ty) -> ky: (0,0) none, (0,1) 1, (1,0) 2, (1,1) 0 and the same for (b, tx) -> kx.  planted: w read as [Co][Ci]"""
    Ci, Co = w.shape[:2]
    if planted:
        w = w.reshape(Co, Ci, 3, 3).permute(1, 0, 2, 3)
    tap = {(0, 0): None, (0, 1): 1, (1, 0): 2, (1, 1): 0}
    o = torch.zeros(4, Co, 4, Ci, dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    ky, kx = tap[(a, ty)], tap[(b, tx)]
                    if ky is not None and kx is not None:
                        o[2 * a + b, :, 2 * ty + tx, :] = w[:, :, ky, kx].t()
    return o


def convT_by_phases(x, wp):
    """the implicit GEMM's phase form as plain torch: x [N, Ci, H, W], wp [4][Co][4][Ci] -> [N, Co, 2H, 2W]; tap (ty, tx) of phase (a, b)
    reads source pixel (i + a - 1 + ty, j + b - 1 + tx), zeros outside the map"""
    N, Ci, H, W = x.shape
    Co = wp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(N, Co, 2 * H, 2 * W, dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            acc = torch.zeros(N, Co, H, W, dtype=x.dtype)
            for ty in (0, 1):
                for tx in (0, 1):
                    src = xp[:, :, a + ty:a + ty + H, b + tx:b + tx + W]
                    acc = acc + torch.einsum("nchw,oc->nohw", src, wp[2 * a + b, :, 2 * ty + tx, :].to(x.dtype))
            out[:, :, a::2, b::2] = acc
    return out


def nhwc(x_nchw, dtype=torch.float16):
    return x_nchw.permute(0, 2, 3, 1).to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------------------- per-kernel references
def _store16(ref, err):
    """bound after one fp16 round-to-nearest of a value known to err"""
    return err + 2.0 ** -11 * (ref.abs() + err) + 2.0 ** -25


def stem_ref(frames_u8, w, bgr=False, zero_pad=False):
    """w [64, 3, 7, 7] (fp32 values) -> (ref, bound) [N, 64, H, W]: 147 taps, one more rounding per term for x / 255"""
    x = frames_u8.permute(0, 3, 1, 2).double()
    if bgr:
        x = x.flip(1)
    x = x / 255.0
    xp = F.pad(x, (3, 3, 3, 3)) if zero_pad else reflect_pad(x, 3)
    k = w.double()
    ref = F.conv2d(xp, k)
    mag = F.conv2d(xp, k.abs())
    return ref, _store16(ref, (148 + 8) * EPS * mag)


def in_stats_ref(x16):
    """x16 [N, C, H, W] fp16 values -> (sum, sum bound, sumsq, sumsq bound), each [N, C]"""
    x = x16.double()
    hw = x.shape[2] * x.shape[3]
    s, q = x.sum(dim=(2, 3)), (x * x).sum(dim=(2, 3))
    return s, (hw + 8) * EPS * x.abs().sum(dim=(2, 3)) + 2.0 ** -140, q, (hw + 9) * EPS * q + 2.0 ** -140


def in_apply_ref(x16, stats, relu, res16=None, unbiased=False):
    """x16 [N, C, H, W] fp16 values, stats [N, C, 2] fp32 values (exact inputs: the sums the kernel was given) -> (ref, bound) [N, C, H, W].
    fp32 arithmetic: mean and sumsq / HW two roundings each, the variance's subtraction against its operands, rsqrt a few ulp, the
    normalised value three roundings, the residual add one; then the fp16 store"""
    x = x16.double()
    hw = float(x.shape[2] * x.shape[3])
    s, q = stats[..., 0].double()[:, :, None, None], stats[..., 1].double()[:, :, None, None]
    mean = s / hw
    e2 = q / hw
    var = (e2 - mean * mean).clamp_min(0)
    if unbiased:
        var = var * hw / max(hw - 1, 1)
    rstd = 1 / torch.sqrt(var + IN_EPS)
    dmean = 3 * EPS * mean.abs()
    dvar = 6 * EPS * (e2 + mean * mean) + 2 * mean.abs() * dmean
    drel = dvar / (2 * (var + IN_EPS)) + 2.0 ** -21
    y = (x - mean) * rstd
    err = y.abs() * (drel + 3 * EPS) + dmean * rstd * (1 + drel)
    if relu:
        y = F.relu(y)
    if res16 is not None:
        y = y + res16.double()
        err = err + EPS * (y.abs() + err)
    return y, _store16(y, err)


def head_ref(xp16, w, b):
    """xp16 [N, 64, H + 6, W + 6] fp16 values (already reflect-padded), w [1, 64, 7, 7], b [1] fp32 values -> (logit, bound) [N, H, W]"""
    x, k = xp16.double(), w.double()
    ref = F.conv2d(x, k, b.double())[:, 0]
    mag = F.conv2d(x.abs(), k.abs(), b.double().abs())[:, 0]
    return ref, (3136 + 1 + 8) * EPS * mag


def conv_valid_ref(xp16, w16):
    """valid 3x3 over a padded map: (ref, mag) [N, Co, H, W]"""
    return F.conv2d(xp16.double(), w16.double()), F.conv2d(xp16.double().abs(), w16.double().abs())


def convT_ref(x16, w16):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) on fp16-rounded operands: (ref, mag) [N, Co, 2H, 2W]"""
    kw = dict(stride=2, padding=1, output_padding=1)
    return F.conv_transpose2d(x16.double(), w16.double(), **kw), F.conv_transpose2d(x16.double().abs(), w16.double().abs(), **kw)
