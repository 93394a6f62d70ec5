"""Every kernel form of the attention family (csrc/attention.hip, csrc/attention_d64.hip), pinned by its kernel symbol, at its tile,
ring and mask edges.

FORMS (tests/attn_forms.py) is the record of what the suite covers: one row per kernel form -- the `prof_symbol` string the launch
records, how the dispatcher is brought to it, and the edge cases run on it.  Every case runs inside ops.Profiler() and FAILS (it is not
skipped) when another kernel than its row names ran: a retuned rung of flash_attn_launch has to update the table in the same commit.

Rungs of flash_attn_launch / op_flash_attn_d64, all in the table:
  D = 40 | 80 | 160                                   -> flash_attn_kernel<D, 4, true, FOLD>       FOLD = k_prescaled
  D = 64, Lq < 2048 (or CTRL_ATTN_NW4 set)            -> flash_attn_kernel<64, 4, true, FOLD>
  D = 64, Lq >= 2048                                  -> flash_attn_kernel<64, 8, false, FOLD>     FOLD = true only where no variant applies
                                                         (Lk % 64 != 0, Lk < 128, kvB == 1) or with variant 0
  D = 64, Lq >= 2048, k_prescaled, Lk % 64 == 0,      -> variants 1 .. 14 of op_flash_attn_d64: flash_attn_d64_kernel<QB, NW, OPT, NSTAGE>
      Lk >= 128, kvB == B                                (12 forms) and flash_attn_d64p_kernel<OPT> (variants 9, 10)
Not in the table: none.  (Other head dims are refused by the dispatcher; test_gpu_ops.py::test_flash_attn_d64_variants holds that an
unknown variant is refused.)  The temporal kernel (temporal_attn_kernel<16 | 32>) has no dispatcher beyond F <= 16; it is run below at
its frame and item-count edges (its launch records the bare kernel name: the frame count in the shape note stands for the template argument).

Three checks per case:

1. the element-wise bound of tests/helpers.py (attn_reference / assert_attn_close) against an fp64 CPU reference over the same fp16
   operands -- derived from the number formats, no measured slack -- and, beside it, the suite's per-tensor rel_inf <= 2e-3.  In the
   folded form the reference is built from the ROUNDED pre-scaled K with scale 1 in the exp2 domain: K is rounded once, as in the plans.
2. inputs that make the edges observable: a key of the last tile spiked against one query (the rescale path) and a key of the first tile
   against another; for every form a negative-offset problem (every true score near -24 in the exp2 domain: a phantom key of score 0 --
   the zero-page K row a wrong mask admits -- would take nearly all the weight, and the first tile is all-negative: the folded form's
   forced first update); V^T pad columns [Lk, roundup8(Lk)) of +-60000 (masked probabilities must be exactly 0) and NaN from there to Lkpad.
3. poisoned surroundings (helpers.Guarded): Q and K are thirds of [rows + guard][3 C + 8] rows with NaN pad columns and NaN guard rows, V^T is
   followed by NaN rows, O lives at ldo = C + 12 (ldo % 4, 8-byte aligned) between guard rows whose fixed bit pattern must come back bit
   for bit.  A finite output proves that no pad reached a kept accumulator.

Grouped launches (ctrl_op_flash_attn_group): a group of three distinct problems must be ONE launch and bit-identical to the three single
launches; a group whose members disagree in Lk falls back to three launches and still matches.
"""
import pytest
import torch

from attn_forms import (ALL, D64_VARIANTS, DEFAULT_VARIANT, F16, TEMPORAL_F, TEMPORAL_ITEMS, C, classic, dispatch, make_problem,
                        temporal_problem)
from helpers import Guarded, _bits, assert_attn_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _attn_launches(prof):
    return [(rec[0], rec[1], rec[2]) for rec in prof.launches if rec[0] not in ("fill_zero", "fill")]


def _check_surroundings(P, what):
    for nm, gd in (("Q", P.Q), ("K", P.K), ("Vt", P.Vt), ("out", P.O)):
        gd.assert_untouched("%s: %s" % (what, nm))


def run_case(ops, gpu, sym, c):
    P = make_problem(ops, gpu, c)
    with dispatch(ops, c):
        with ops.Profiler() as prof:
            ops.flash_attn(*P.args, **P.kw)
        torch.cuda.synchronize()
    launches = _attn_launches(prof)
    print("FORM %-44s ran %-44s %s" % (c.name, " + ".join(l[1] or l[0] for l in launches), launches[0][2] if launches else ""))
    assert len(launches) == 1 and launches[0][0] == "flash_attn" and launches[0][1] == sym, "%s: expected %s, the dispatcher launched %s" % (
        c.name, sym, launches)
    what = "%s [%s]" % (c.name, sym)
    _check_surroundings(P, what)
    return assert_attn_close(P.O.view, P.ref, P.bound, what)


@pytest.mark.parametrize("idx", range(len(ALL)), ids=[c.name.replace(" ", "_") for _, _, c in ALL])
def test_form(ops, gpu, idx):
    sym, how, c = ALL[idx]
    run_case(ops, gpu, sym, c)


# ------------------------------------------------------------------------------------------------------------------------------------
# grouped launches
# ------------------------------------------------------------------------------------------------------------------------------------
_w8 = dict(D=64, Lq=2085, B=2, heads=5)
GROUPS = [
    (classic(64, 4, True, True), C("group classic 4-wave", D=64, fold=True, Lq=129, Lk=77)),
    (classic(64, 8, False, False), C("group classic 8-wave", fold=False, Lk=77, **_w8)),
    (D64_VARIANTS[DEFAULT_VARIANT][0], C("group d64 default variant", fold=True, Lk=192, **_w8)),
    (D64_VARIANTS[9][0], C("group d64p", fold=True, Lk=192, variant=9, **_w8)),
]


def _desc(ops, P):
    kw = dict(P.kw)
    return ops.flash_attn_desc(*P.args, kw.pop("out"), kw.pop("ldo"), **kw)


def _run_group(ops, gpu, sym, cases, one_launch):
    """three single launches, then the same three problems (fresh outputs) as a group: bit-identical, guards intact, and the profiler shows
    one launch of three (or, for members that disagree, three launches)"""
    prev = ops.set_policy("CTRL_GROUP", "1")
    try:
        with dispatch(ops, cases[0]):
            singles = [make_problem(ops, gpu, c, seed=11 + i) for i, c in enumerate(cases)]
            for P in singles:
                ops.flash_attn(*P.args, **P.kw)
            grouped = [make_problem(ops, gpu, c, seed=11 + i) for i, c in enumerate(cases)]
            with ops.Profiler() as prof:
                ops.flash_attn_group([_desc(ops, P) for P in grouped])
            torch.cuda.synchronize()
    finally:
        ops.set_policy("CTRL_GROUP", prev)
    launches = _attn_launches(prof)
    print("FORM %-44s ran %-44s %s" % (cases[0].name, " + ".join(l[1] for l in launches), " | ".join(l[2] for l in launches)))
    assert all(l[0] == "flash_attn" and l[1] == sym for l in launches), (sym, launches)
    if one_launch:
        assert len(launches) == 1 and launches[0][2].endswith(" x3"), launches
    else:
        assert len(launches) == 3 and all(" x" not in l[2] for l in launches), launches
    for i, (S, G) in enumerate(zip(singles, grouped)):
        what = "%s member %d [%s]" % (cases[i].name, i, sym)
        _check_surroundings(S, what + " single")
        _check_surroundings(G, what + " grouped")
        assert torch.equal(_bits(S.O.view), _bits(G.O.view)), "%s: the grouped result differs from the single launch" % what
        assert_attn_close(G.O.view, G.ref, G.bound, what)
    assert not torch.equal(grouped[0].O.view, grouped[1].O.view)        # (distinct problems: a member served from a sibling's data would show)


@pytest.mark.parametrize("idx", range(len(GROUPS)), ids=[c.name.replace(" ", "_") for _, c in GROUPS])
def test_group_of_three_is_one_launch_and_bit_identical(ops, gpu, idx):
    sym, c = GROUPS[idx]
    _run_group(ops, gpu, sym, [c, c, c], one_launch=True)


def test_group_whose_members_disagree_falls_back_to_single_launches(ops, gpu):
    sym, c = GROUPS[0]
    other = C(c.name + " Lk65", **{**{k: v for k, v in c.items() if k != "name"}, "Lk": 65})
    _run_group(ops, gpu, sym, [c, other, c], one_launch=False)


# ------------------------------------------------------------------------------------------------------------------------------------
# temporal attention
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bc,HW,heads", TEMPORAL_ITEMS, ids=["items%d" % (a * b * c) for a, b, c in TEMPORAL_ITEMS])
@pytest.mark.parametrize("Fr", TEMPORAL_F)
def test_temporal_form(ops, gpu, Fr, Bc, HW, heads):
    """temporal_attn_kernel<16 | 32> at F in {1, 2, 15, 16, 17, 31, 32} and at item counts that leave 3, 1 and 3 waves of the last workgroup
    dead; q | k | v rows at ld = 3 C + 8 with NaN pads and guard rows, O at ldo = C + 8 between guard rows; the same bound without its
    P-rounding term (this kernel keeps P in fp32)"""
    Cc = heads * 64
    rows = Bc * Fr * HW
    qkv, ref, bound = temporal_problem(Bc, Fr, HW, heads)
    X = Guarded.inp(qkv.half(), (3, 0), (5, 8), gpu)
    O = Guarded.out((2 + rows + 6, Cc + 8), (slice(2, 2 + rows), slice(0, Cc)), F16, gpu)
    with ops.Profiler() as prof:
        ops.temporal_attn(X.view, Bc, Fr, HW, heads, out=O.view, ldo=Cc + 8)
    torch.cuda.synchronize()
    launches = _attn_launches(prof)
    sym = "temporal_attn_kernel"                 # (<16> for F <= 16, else <32>: the launch records the bare name, and F in its shape note)
    name = "temporal F%d items%d" % (Fr, Bc * HW * heads)
    print("FORM %-44s ran %-44s %s" % (name, " + ".join(l[1] or l[0] for l in launches), launches[0][2] if launches else ""))
    assert len(launches) == 1 and launches[0][0] == "temporal_attn" and launches[0][1] == sym and " F%d " % Fr in launches[0][2], (name, sym, launches)
    what = "%s [%s]" % (name, sym)
    X.assert_untouched(what + ": qkv")
    O.assert_untouched(what + ": out")
    assert_attn_close(O.view, ref, bound, what)
