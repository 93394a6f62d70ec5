"""The small 3x3 convolutions (csrc/smallconv.hip) at their edges: case tables, fp64 reference, element-wise bound and the guarded placement.

    GPU tests and the host section (tables, refusals): tests/test_gpu_smallconv_forms.py

conv3x3_direct_kernel has five template forms (NCHW in of any dtype, channels-last fp16 in, both with fp16 rows out; the two fp32 stems --
NCHW in / fp32 rows in, fp32 rows out -- which write the residual stream of the backbone UNets), each with 16 or 32 output channels per
thread; conv3x3_small_mfma_kernel has four (Cin, Cout) forms.  Reference: fp64 conv2d (+ SiLU) over the same operand values.  Bound:

    |out - ref| <= (9 Cin + 8) 2^-24 (|x| (*) |w| + |b|)  [x 1.1 through SiLU: |silu'| <= 1.1]  + the rounding of the stored value

an fp32 sum of 9 Cin products and the bias in ANY order (+ 8: the few operations of the activation, whose v_exp_f32 / v_rcp_f32 are good to an
ulp each); fp16 outputs add 2^-11 (|ref| + bound) + 2^-25.  Nothing is measured.
"""
import functools

import torch
import torch.nn.functional as Fn

COUTS = (16, 48, 64)          # one channel block of 16; three of 16; two of 32
# (N, H, W, stride): N Hout Wout = 255, 256, 257 (one thread short of a block, a block, one over); five 9 x 7 images, whose boundaries fall
# inside a thread block; stride 2 on odd and on even H and W; stride 2 over more than one block
SHAPES = ((1, 15, 17, 1), (1, 16, 16, 1), (1, 1, 257, 1), (5, 9, 7, 1), (3, 9, 7, 2), (3, 8, 10, 2), (1, 31, 33, 2))
# direct forms: name -> (op, Cin, input layout, input dtype)
DIRECT_FORMS = {
    "nchw3-f32": ("direct", 3, "nchw", torch.float32), "nchw3-f16": ("direct", 3, "nchw", torch.float16), "nchw3-bf16": ("direct", 3, "nchw", torch.bfloat16),
    "nchw4-f32": ("direct", 4, "nchw", torch.float32), "nchw4-f16": ("direct", 4, "nchw", torch.float16), "nchw4-bf16": ("direct", 4, "nchw", torch.bfloat16),
    "nhwc16": ("direct", 16, "nhwc", torch.float16), "nhwc32": ("direct", 32, "nhwc", torch.float16),
    "stem4-f32": ("stem", 4, "nchw", torch.float32), "stem4-f16": ("stem", 4, "nchw", torch.float16),
    "stem8-f32": ("stem", 8, "nchw", torch.float32), "stem8-f16": ("stem", 8, "nchw", torch.float16),
    "rows8": ("rows", 8, "nhwc", torch.float32),
}


def _direct_table():
    out = []
    for fi, (name, (op, cin, layout, dt)) in enumerate(DIRECT_FORMS.items()):
        for si, (N, H, W, stride) in enumerate(SHAPES):
            if op != "direct" and stride != 1:
                continue          # the stems are stride 1, no activation
            out.append(dict(id="%s-n%d-%dx%d-s%d" % (name, N, H, W, stride), form=name, op=op, Cin=cin, layout=layout, dtype=dt, N=N, H=H, W=W,
                            stride=stride, Cout=COUTS[(si + fi) % 3], bias=(si + fi) % 4 != 0, silu=op == "direct" and (si + fi) % 2 == 1,
                            seed=4000 + 31 * fi + si))
    return out


DIRECT_CASES = _direct_table()

# MFMA kernel: every (Cin, Cout) pair x (stride, Hin, Win): Hout in {7, 8, 9, 17} around the 8-row unit, Wout in {15, 16, 17, 33} around the
# 16-pixel fragment; stride 2 on odd and on even sizes
MFMA_GEOMS = ((1, 7, 15), (1, 8, 16), (1, 9, 17), (1, 17, 33), (2, 17, 33), (2, 16, 32), (2, 13, 29), (2, 34, 66))


def _mfma_table():
    out = []
    for pi, (cin, cout) in enumerate(((16, 16), (16, 32), (32, 16), (32, 32))):
        for gi, (stride, H, W) in enumerate(MFMA_GEOMS):
            out.append(dict(id="mfma%d-%d-%dx%d-s%d" % (cin, cout, H, W, stride), form="mfma%d-%d" % (cin, cout), op="mfma", Cin=cin, Cout=cout,
                            layout="nhwc", dtype=torch.float16, N=2, H=H, W=W, stride=stride, bias=(gi + pi) % 2 == 0, silu=False,
                            seed=5000 + 31 * pi + gi))
    return out


MFMA_CASES = _mfma_table()
CASE_BY_ID = {c["id"]: c for c in DIRECT_CASES + MFMA_CASES}


def out_hw(c):
    return (c["H"] - 1) // c["stride"] + 1, (c["W"] - 1) // c["stride"] + 1


@functools.lru_cache(maxsize=None)
def problem(case_id):
    """x [N][Cin][H][W] in the case's input dtype (fp32 inputs are NOT fp16-representable), w [Cout][Cin][3][3] (fp16 values for the MFMA
    kernel, which both kernels then read), b [Cout] | None"""
    c = CASE_BY_ID[case_id]
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn(c["N"], c["Cin"], c["H"], c["W"], generator=g).to(c["dtype"])
    w = torch.randn(c["Cout"], c["Cin"], 3, 3, generator=g) * 0.2
    if c["op"] == "mfma":
        w = w.half().float()
    b = torch.randn(c["Cout"], generator=g) * 0.5 if c["bias"] else None
    return x, w, b


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(ref, bound) as [N][Hout][Wout][Cout] fp64, for the case's output format"""
    c = CASE_BY_ID[case_id]
    x, w, b = problem(case_id)
    xd, wd = x.double(), w.double()
    pre = Fn.conv2d(xd, wd, b.double() if b is not None else None, stride=c["stride"], padding=1)
    mag = Fn.conv2d(xd.abs(), wd.abs(), b.double().abs() if b is not None else None, stride=c["stride"], padding=1)
    bound = (9 * c["Cin"] + 8) * 2.0 ** -24 * mag
    ref = pre
    if c["silu"]:
        ref, bound = pre * torch.sigmoid(pre), 1.1 * bound
    if c["op"] in ("direct", "mfma"):          # fp16 rows out
        bound = bound + 2.0 ** -11 * (ref.abs() + bound) + 2.0 ** -25
    return ref.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


PAD = 64          # guard elements in front of and behind every operand (a multiple of 16 bytes in every dtype)


def place(case_id, device, ops, kernel=None):
    """the case on the GPU, every operand inside a guarded allocation; kernel: "direct" runs an MFMA case on the direct kernel.
    Returns dict(x, w, b, out: Guarded (b: | None), run: a callable that launches)"""
    from helpers import Guarded
    c = CASE_BY_ID[case_id]
    x, w, b = problem(case_id)
    op = kernel or c["op"]
    Ho, Wo = out_hw(c)
    xin = x if c["layout"] == "nchw" else x.permute(0, 2, 3, 1).contiguous()
    gx = Guarded.inp(xin.reshape(-1), (PAD,), (PAD,), device)
    xv = gx.view.view(xin.shape)
    wp = (ops.pack_conv_w if op == "mfma" else ops.pack_conv_w_direct)(w.to(device))
    gw = Guarded.inp(wp.reshape(-1), (PAD,), (PAD,), device)
    gb = Guarded.inp(b, (PAD,), (PAD,), device) if b is not None else None
    odt = torch.float32 if op in ("stem", "rows") else torch.float16
    n_out = c["N"] * Ho * Wo * c["Cout"]
    go = Guarded.out((n_out + 2 * PAD,), (slice(PAD, PAD + n_out),), odt, device)
    ov = go.view.view(c["N"], Ho, Wo, c["Cout"])
    bv = gb.view if gb is not None else None
    if op == "direct":
        run = lambda: ops.conv3x3_direct(xv, gw.view, bv, c["Cout"], stride=c["stride"], silu=c["silu"], nchw=c["layout"] == "nchw", out=ov)      # noqa: E731
    elif op == "mfma":
        run = lambda: ops.conv3x3_small_mfma(xv, gw.view, bv, c["Cout"], stride=c["stride"], silu=c["silu"], out=ov)      # noqa: E731
    elif op == "stem":
        run = lambda: ops.conv3x3_direct_f32(xv, gw.view, bv, c["Cout"], out=ov)      # noqa: E731
    else:
        run = lambda: ops.conv3x3_rows_f32(xv, gw.view, bv, c["Cout"], out=ov)      # noqa: E731
    return dict(case=c, x=gx, w=gw, b=gb, out=go, out_view=ov, run=run)


def guards(q):
    return [g for g in (q["x"], q["w"], q["b"], q["out"]) if g is not None]
