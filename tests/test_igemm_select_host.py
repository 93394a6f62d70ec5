"""Which kernel form the implicit GEMM selects (csrc/igemm.hip: igemm_select), checked without a GPU.

ctrl_igemm_select answers from the descriptor, the policy table and the test overrides alone, so every row of the forms table
(tests/igemm_forms.py: FORMS, SPLITK -- the table tests/test_gpu_igemm_forms.py launches) is asked here over CPU tensors of the same
shapes, paddings and pointer alignments, under the case's policy and `wide` setting: the selector must name the row's kernel symbol,
and for a split-K row the split count and the reduction of each of the three `reduce` variants.  A retuned threshold fails here, on
the build machine, before any launch."""
import pytest
import torch

from igemm_forms import ALL, F16, ROWS, SPLITK, C, attach_splitk, case_policy, make_problem, ring, splitk_variant, wide8

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def ops():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def select(ops, c, group_n=1):
    P = make_problem(ops, CPU, c, reference=False)
    with case_policy(ops, c):
        if c.splitk:
            attach_splitk(ops, CPU, c, P)
        return ops.igemm_select(ops.igemm_desc(**P.kw), group_n, pinned=bool(c.pinned))


@pytest.mark.parametrize("idx", range(len(ALL)), ids=[c.name.replace(" ", "_") for _, _, c in ALL])
def test_form_is_selected(ops, idx):
    sym, how, c = ALL[idx]
    got = select(ops, c)
    assert got == sym, "%s (%s): expected %s, the selector names %s" % (c.name, how, sym, got)


@pytest.mark.parametrize("reduce", ["finish", "inlaunch", "inlaunch_tickets"])
@pytest.mark.parametrize("idx", range(len(SPLITK)), ids=[c.name.replace(" ", "_") for _, c in SPLITK])
def test_splitk_form_is_selected(ops, idx, reduce):
    sym, c = SPLITK[idx]
    c = splitk_variant(sym, c, reduce)
    want = "%s splitk%d%s" % (sym, c.sk, " in-launch" if c.splitk == "inlaunch" else "")
    got = select(ops, c)
    assert got == want, "%s [%s]: expected %r, the selector names %r" % (c.name, reduce, want, got)


# The forms table stands ON every threshold of the ladder (the first tile count that takes a form); these rows stand one tile (one row)
# BELOW it and name what the ladder falls through to, so that a threshold moved in either direction fails on the build machine.
BELOW = [
    (ring(64, 64, 64, 2, 2, 3, ROWS), C("below 512 tiles of 128^2 (small-tile policy): 127 x 4", mode=ROWS, M=127 * 128, Nout=512, Cin=64, res=F16)),
    (ring(64, 64, 32, 2, 2, 3, ROWS), C("below 192 tiles of 128^2 (Cin % 64 != 0): 47 x 4", mode=ROWS, M=47 * 128, Nout=512, Cin=96, res=F16)),
    (ring(128, 128, 32, 2, 2, 3, ROWS), C("below 200 tiles of 256 x 256: 199 x 1", mode=ROWS, M=199 * 256, Nout=256, Cin=64, res=F16)),
    (ring(128, 128, 32, 2, 2, 3, ROWS), C("below 160 tiles of 256 x 320: 159 x 1", mode=ROWS, M=159 * 256, Nout=320, Cin=64, res=F16)),
    (wide8(4, ROWS), C("below M = 65536 (the two-workgroup tiles of the stream updates)", mode=ROWS, M=65535, Nout=256, Cin=64, res=F16)),
]


@pytest.mark.parametrize("idx", range(len(BELOW)), ids=[c.name.replace(" ", "_") for _, c in BELOW])
def test_one_below_a_threshold(ops, idx):
    sym, c = BELOW[idx]
    got = select(ops, c)
    assert got == sym, "%s: expected %s, the selector names %s" % (c.name, sym, got)


def test_grouped_selection(ops):
    """four problems of 32 x 4 tiles of 128^2 each: alone below the small-tile policy's 512 tiles (64 x 64 x 64), as a group of four at
    them (128 x 128 x 32); with ctrl_group_launches(2) the group selects what the problem gets alone"""
    c = C("grouped rows M4096", mode=ROWS, M=4096, Nout=512, Cin=64, res=F16)
    alone, grouped = ring(64, 64, 64, 2, 2, 3, ROWS), ring(128, 128, 32, 2, 2, 3, ROWS)
    assert ops.set_group_launches(None) == 1
    assert select(ops, c) == alone
    assert select(ops, c, group_n=4) == grouped
    try:
        assert ops.set_group_launches(2) == 2
        assert select(ops, c, group_n=4) == alone
    finally:
        ops.set_group_launches(1)


def test_pinned_form_is_refused_where_it_does_not_apply(ops):
    c = C("pinned Cin 96", mode=ROWS, M=65, Nout=64, Cin=96, pinned=True)
    with pytest.raises(RuntimeError, match="igemm_pinned"):
        select(ops, c)
