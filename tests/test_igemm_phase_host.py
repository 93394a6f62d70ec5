"""The phase form of the implicit GEMM (csrc/igemm.hip: IG_CONV2D_PHASE) without a GPU: what the selector names for it
(ctrl_igemm_select over CPU tensors) and what the validation refuses."""
import pytest
import torch

from igemm_forms import F16, case_policy, ring, wide8
from igemm_phase_cases import CASES, GROUPS, PHASE, make_phase_problem, phase_contract, phase_pack

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def ops():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _desc(ops, n, H, W, Cin, Nout, keep, **over):
    """a phase descriptor over small aligned CPU tensors (the selector reads shapes, strides and pointer alignments, never the data)"""
    t = torch.zeros(64, dtype=F16)
    b = torch.zeros(64, dtype=torch.float32)
    keep += [t, b]
    kw = dict(A=t, lda=Cin, W=t, M=n * 4 * H * W, Nout=Nout, Cin=Cin, taps=4, mode=PHASE,
              geom=dict(Hin=H, Win=W, Hout=2 * H, Wout=2 * W, stride=1, up=2), bias=b, rowvec=b, rows_per_img=4 * H * W,
              segs=[(t, Nout, 0, Nout, ops.SEG_ROW, 1)])
    kw.update(over)
    return ops.igemm_desc(**kw)


# conv1 of the SDXL adapter's up-sampling ResNets at batch 8 (bench.py): locations A, B, C as groups of 3, 2, 2 sibling blocks
STEP = [("A", 64, 320, 3), ("B", 32, 640, 2), ("C", 16, 1280, 2)]


@pytest.mark.parametrize("loc,h,ch,group", STEP, ids=[s[0] for s in STEP])
def test_step_shapes_take_the_wide_phase_tile(ops, loc, h, ch, group):
    keep = []
    d = _desc(ops, 8, h, h, ch, ch, keep)
    got = ops.igemm_select(d, group)
    assert got == wide8(5, PHASE), "location %s: the selector names %s" % (loc, got)       # never split-K: no " splitkN" suffix
    assert ops.igemm_splitk_plan(_desc(ops, 8, h, h, ch, ch, keep, splitk_ws=torch.zeros(64)))[0] == 1


@pytest.mark.parametrize("idx", range(len(CASES) + len(GROUPS)), ids=[c.name.split(":")[0].replace(" ", "_") for c in CASES + GROUPS])
def test_case_shapes_select_their_form(ops, idx):
    c = (CASES + GROUPS)[idx]
    P = make_phase_problem(ops, CPU, c, reference=False)
    with case_policy(ops, c):
        got = ops.igemm_select(ops.igemm_desc(**P.kw), 3 if idx >= len(CASES) else 1)
    assert got == c.sym, "%s: expected %s, the selector names %s" % (c.name, c.sym, got)


def test_few_tile_shapes_fall_to_the_ring_tiles(ops):
    keep = []
    assert ops.igemm_select(_desc(ops, 1, 1, 1, 64, 64, keep)) == ring(64, 64, 64, 2, 2, 3, PHASE)
    assert ops.igemm_select(_desc(ops, 2, 8, 8, 320, 320, keep)) == ring(64, 64, 64, 2, 2, 3, PHASE)
    # one tile below / at the wide tile's 160: 4 phases x 39 | 40 tiles of 256 rows x 1 column of 320
    assert ops.igemm_select(_desc(ops, 1, 39 * 16, 16, 64, 320, keep)) == ring(128, 128, 64, 2, 4, 4, PHASE)
    assert ops.igemm_select(_desc(ops, 1, 40 * 16, 16, 64, 320, keep)) == wide8(5, PHASE)


def test_validation_refuses_what_the_form_does_not_cover(ops):
    keep = []
    r = torch.zeros(64, dtype=F16)
    for what, over in (("a split operand", dict(a_split=2, Cin=128)), ("a residual", dict(res=r, ldres=64)), ("nine taps", dict(taps=9)),
                       ("a transposed output", dict(segs=[(r, 64, 0, 64, 1, 64)])), ("Cin % 64 != 0", dict(Cin=96))):
        with pytest.raises(RuntimeError, match="phase form"):
            ops.igemm_select(_desc(ops, 1, 4, 4, over.pop("Cin", 64), 64, keep, **over))
        print("refused:", what)
    with pytest.raises(RuntimeError, match="phase form"):          # Hout != 2 Hin
        ops.igemm_select(_desc(ops, 1, 4, 4, 64, 64, keep, geom=dict(Hin=4, Win=4, Hout=4, Wout=8, stride=1, up=2)))


def test_phase_assembly_equals_the_conv_of_the_upsampled_map():
    """the arithmetic behind the form, in fp64: four 2x2 convolutions with the summed weights == conv2d(nearest x2 (x), w, padding 1)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 7, 8, generator=g, dtype=torch.float64)
    w = torch.randn(6, 8, 3, 3, generator=g, dtype=torch.float64)
    wp = torch.zeros(4, 6, 4, 8, dtype=torch.float64)
    from igemm_phase_cases import TAPS
    for a in (0, 1):
        for b in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    wp[2 * a + b, :, 2 * ty + tx, :] = sum(w[:, :, ky, kx] for ky in TAPS[(a, ty)] for kx in TAPS[(b, tx)])
    up = x.permute(0, 3, 1, 2).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ref = torch.nn.functional.conv2d(up, w, padding=1).permute(0, 2, 3, 1)
    got = phase_contract(x, wp)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-13
    # and the pack the tests hold the device kernel against is these sums, taken in fp32
    assert float((phase_pack(w.float()).double() - wp).abs().max()) < 1e-5
