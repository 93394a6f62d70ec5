"""The pure-data part of tests/test_gpu_igemm_phase.py: the phase form of the implicit GEMM (csrc/igemm.hip: IG_CONV2D_PHASE) -- a 3x3
convolution (padding 1) over a nearest x2 up-sampled map computed as four 2x2 convolutions over the SOURCE map, one per output phase
(oy & 1, ox & 1).  The CPU phase pack, the cases, and the construction of a case's operands and descriptor on a given device; the
selection test that needs no GPU (tests/test_igemm_phase_host.py) builds the same descriptors over CPU tensors."""
import types

import torch
import torch.nn.functional as F

from helpers import Guarded
from igemm_forms import F16, F32, Case, _gen, _h, ring, wide8

PHASE = 3                                               # ctrl_igemm_desc::mode
TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # S(a, ty): the 3x3 rows (columns) behind tap ty (tx) of phase a (b)


def phase_pack(w9):
    """[Cout][Cin][3][3] fp32 -> fp32 [4 phases][Cout][4 taps][Cin]: the tap sums in fp32, in (ky, kx) order, NOT yet rounded"""
    w9 = w9.float()
    cout, cin = w9.shape[:2]
    out = torch.zeros(4, cout, 4, cin, dtype=torch.float32)
    for a in (0, 1):
        for b in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    s = None
                    for ky in TAPS[(a, ty)]:
                        for kx in TAPS[(b, tx)]:
                            s = w9[:, :, ky, kx].clone() if s is None else s + w9[:, :, ky, kx]      # one fp32 addition per term
                    out[2 * a + b, :, 2 * ty + tx, :] = s
    return out


def phase_contract(x, wp):
    """fp64 reference of the phase GEMM: x [n][H][W][Cin], wp [4][Cout][4][Cin] (both fp64) -> [n][2H][2W][Cout].  Tap (ty, tx) of phase
    (a, b) reads source pixel (i + a - 1 + ty, j + b - 1 + tx), zero outside the map"""
    n, H, W, _ = x.shape
    cout = wp.shape[1]
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = torch.zeros(n, 2 * H, 2 * W, cout, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            k = wp[2 * a + b].reshape(cout, 2, 2, -1).permute(0, 3, 1, 2)          # [Cout][Cin][ty][tx]
            y = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k)                     # padded row i + a + ty = source row i + a - 1 + ty
            out[:, a::2, b::2, :] = y.permute(0, 2, 3, 1)
    return out


def C(name, sym, **kw):
    return Case(name=name, sym=sym, **kw)


# The smallest shapes at which each piece can go wrong.  `sym`: the kernel the dispatcher must name; wide=2: ops.set_igemm_wide(2), every
# eligible problem on the 8-phase wide tile (how the suite runs small shapes through it); pad=12: ld % 8 != 0 -> the scalar epilogue.
R64, R64S = ring(64, 64, 64, 2, 2, 3, PHASE), ring(64, 64, 64, 2, 2, 3, PHASE, swap=False)
CASES = [
    C("1x1: every tap but one per phase is padding", R64, n=1, H=1, W=1, Cin=64, Nout=64),
    C("5x7: ragged phases of 70 rows, one k-tile per tap, all four borders", R64, n=2, H=5, W=7, Cin=64, Nout=64),
    C("5x7 scalar epilogue (ld % 8 != 0)", R64S, n=2, H=5, W=7, Cin=64, Nout=64, pad=12),
    C("8x8 wide5: 192 rows per phase below BM, fp32 + mirror, per-image rowvec", wide8(5, PHASE), n=3, H=8, W=8, Cin=128, Nout=320, wide=2,
      out=F32, mirror=True),
    C("8x8 wide4: phases of exactly one 256-row tile", wide8(4, PHASE), n=4, H=8, W=8, Cin=64, Nout=256, wide=2),
    C("33x31: several tiles per phase, ragged last one, default selection", R64, n=1, H=33, W=31, Cin=64, Nout=320),
    # the other two ring tiles the ladder can reach: 4 phases x 12 tiles x 4 columns = 192 tiles of 128^2; 4 x 16 x 3 = 192 tiles of 128 x 64
    C("23x22 Nout 512: 128x128x64, 12 tiles per phase, ragged", ring(128, 128, 64, 2, 4, 4, PHASE), n=3, H=23, W=22, Cin=64, Nout=512),
    C("26x25 Nout 192: 128x64x64, 16 tiles per phase, ragged", ring(128, 64, 64, 2, 2, 3, PHASE), n=3, H=26, W=25, Cin=64, Nout=192, out=F32),
]
GROUPS = [C("group of three 5x7", R64, n=2, H=5, W=7, Cin=64, Nout=64),
          C("group of three 8x8 wide5", wide8(5, PHASE), n=3, H=8, W=8, Cin=128, Nout=320, wide=2, out=F32, mirror=True)]


def make_phase_problem(ops, device, c, seed=0, reference=True):
    """operands of case `c` inside poisoned surroundings on `device` (as tests/igemm_forms.py: make_problem), the ops.igemm keyword
    arguments over them and two fp64 references: (ref, mag) of the phase GEMM over the exact fp16 pack, and ref9 = the 3x3 convolution
    of the up-sampled map with the UNROUNDED fp32 weights"""
    g = _gen(7000 + seed) if reference else None
    rnd = (lambda *shape: torch.randn(*shape, generator=g)) if reference else torch.empty
    n, H, W, Cin, Nout = c.n, c.H, c.W, c.Cin, c.Nout
    odt = c.out or F16
    M = n * 4 * H * W
    x = _h((n, H, W, Cin), g)
    w9 = rnd(Nout, Cin, 3, 3) * 0.05                      # fp32, NOT fp16-representable: the pack sums, then rounds once
    wp16 = phase_pack(w9).half() if reference else torch.empty(4, Nout, 4, Cin, dtype=F16)
    bias, rowvec = rnd(Nout), rnd(n, Nout)
    ref = mag = ref9 = None
    if reference:
        add = (bias.double()[None, :] + rowvec.double())[:, None, None, :]
        madd = (bias.double().abs()[None, :] + rowvec.double().abs())[:, None, None, :]
        ref = (phase_contract(x.double(), wp16.double()) + add).reshape(M, Nout)
        mag = (phase_contract(x.double().abs(), wp16.double().abs()) + madd).reshape(M, Nout)
        up = x.double().permute(0, 3, 1, 2).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)      # nearest x2
        ref9 = (F.conv2d(up, w9.double(), padding=1).permute(0, 2, 3, 1) + add).reshape(M, Nout)
    A = Guarded.inp(x.half(), (1, 0, 0, 0), (1, 0, 0, 8), device)          # NaN guard images before and after, NaN pad columns
    Wg = Guarded.inp(wp16.reshape(4 * Nout, 4 * Cin).contiguous(), (0, 0), (64, 0), device)
    Bg = Guarded.inp(bias, (0,), (64,), device)
    Rv = Guarded.inp(rowvec, (0, 0), (2, 0), device)
    pad = 16 if c.pad is None else c.pad
    O = Guarded.out((M + 64, Nout + pad), (slice(0, M), slice(0, Nout)), odt, device)
    Mir = Guarded.out((M + 64, Nout + 16), (slice(0, M), slice(0, Nout)), F16, device) if c.mirror else None
    kw = dict(A=A.view, lda=Cin + 8, W=Wg.view, M=M, Nout=Nout, Cin=Cin, taps=4, mode=PHASE,
              geom=dict(Hin=H, Win=W, Hout=2 * H, Wout=2 * W, stride=1, up=2), bias=Bg.view, rowvec=Rv.view, rows_per_img=4 * H * W,
              segs=[(O.view, Nout + pad, 0, Nout, ops.SEG_ROW, 1)], out16=Mir.view if Mir else None, ld16=Nout + 16 if Mir else 0)
    return types.SimpleNamespace(kw=kw, A=A, Wg=Wg, Bg=Bg, Rv=Rv, O=O, Mir=Mir, M=M, Nout=Nout, Ktot=4 * Cin, ref=ref, mag=mag, ref9=ref9, w9=w9)
