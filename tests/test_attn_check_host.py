"""No GPU: the table of attention forms (tests/attn_forms.py) is complete and names the tile counts it claims, and the element-wise bound
of tests/helpers.py (attn_reference) holds for a plain fp32 / fp16 emulation of the kernels' arithmetic on the table's own problems."""
import torch

import helpers  # noqa: F401  (puts the repository root on sys.path)
from attn_forms import ALL, D64_VARIANTS, FORMS, TEMPORAL_F, TEMPORAL_ITEMS, classic, emulate, host_problem, temporal_problem, _heads


def test_table_names_every_form_and_every_ring_remainder():
    syms = {sym for sym, _, _ in FORMS}
    want = {classic(D, 4, True, f) for D in (40, 64, 80, 160) for f in (False, True)} | {classic(64, 8, False, f) for f in (False, True)}
    want |= {s for s, _, _ in D64_VARIANTS.values()}
    assert syms == want and len(D64_VARIANTS) == 14 and len(want) == 24
    tiles = {}
    for sym, _, c in ALL:
        tiles.setdefault(sym, set()).add((c.Lk + 63) // 64)
        assert c.kind in ("spike", "neg") and c.Lq >= 1 and c.Lk >= 1
    for v, (sym, qwg, nstage) in D64_VARIANTS.items():
        assert tiles[sym] >= {2, 3, 4, 5, 6, 7}, (v, tiles[sym])
        assert {t % nstage for t in tiles[sym]} == set(range(nstage))
    for sym in want - {s for s, _, _ in D64_VARIANTS.values()}:
        assert tiles[sym] >= ({1, 2, 3, 4, 5} if ", 4, " in sym else {1, 2, 3, 5}), (sym, tiles[sym])
        assert any(c.kvB == 1 for s, _, c in ALL if s == sym), sym
    for sym in want:
        assert any(c.kind == "neg" for s, _, c in ALL if s == sym), sym          # a negative-offset problem for every form
    # d64 applicability as the dispatcher sees it: a case that names a variant > 0 must be admitted, every other Lq >= 2048 folded case not
    for sym, _, c in ALL:
        applies = c.D == 64 and c.fold and c.Lk % 64 == 0 and c.Lk >= 128 and (c.kvB or c.B) == c.B and c.Lq >= 2048
        assert sym.startswith("flash_attn_d64") == bool(applies and c.variant != 0), c.name
    assert {a * b * c for a, b, c in TEMPORAL_ITEMS} == {1, 3, 5, 120} and set(TEMPORAL_F) == {1, 2, 15, 16, 17, 31, 32}


def _emulated(c, thr):
    H = host_problem(c)
    N = c.B * c.heads
    fl = lambda t: _heads(t, c.heads).expand(c.B, -1, -1, -1).reshape(N, t.shape[1], c.D)
    o = emulate(fl(H.q), fl(H.k), fl(H.v), H.c, bool(c.fold), thr)
    return H, o.reshape(c.B, c.heads, c.Lq, c.D).transpose(1, 2).reshape(c.B * c.Lq, c.heads * c.D).double()


def test_bound_holds_for_an_emulation_of_the_kernels_arithmetic():
    """fp32 scores and sums, P rounded to fp16 for P . V, a reference point deferred by 0 / 2^4 / 2^8, an fp16 result: every 4-wave case
    of the table (the long-sequence problems are the same arithmetic at more rows)"""
    worst = 0.0
    for sym, _, c in ALL:
        if c.Lq > 256:
            continue
        for thr in ((0.0, 4.0, 8.0) if c.fold else (0.0,)):
            H, o = _emulated(c, thr)
            assert bool(torch.isfinite(o).all()), c.name
            r = float(((o - H.ref).abs() / H.bound).max())
            worst = max(worst, r)
            assert r <= 1.0, (c.name, thr, r)
    print("ATTN-CHECK emulation: worst err/bound %.3f" % worst)


def test_bound_of_the_temporal_problems_admits_an_fp32_computation():
    qkv, ref, bound = temporal_problem(2, 17, 12, 5)
    assert ref.shape == bound.shape == (2 * 17 * 12, 320) and bool(torch.isfinite(bound).all())
    q = qkv.reshape(2, 17, 12, 3, 5, 64)
    o32 = torch.softmax(torch.einsum("bfphd,bgphd->bphfg", q[:, :, :, 0], q[:, :, :, 1]) / 8.0, -1)
    o32 = torch.einsum("bphfg,bgphd->bfphd", o32, q[:, :, :, 2]).reshape(2 * 17 * 12, 320).half().double()
    assert bool(((o32 - ref).abs() <= bound).all())
