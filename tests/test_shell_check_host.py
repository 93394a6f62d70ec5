"""Self-test of the shell-kernel checks (tests/shell_forms.py), no GPU: the tables hold the edges they declare (asserted from constants
restated from csrc/vae.hip and csrc/unet.hip), the fp32 emulations of the kernels stay within the bounds (at most 0.5 of them where a
constant was calibrated, and above 0.5 one power of two lower), every planted error is rejected on a named case, the encoder's fp64
restatement agrees with tests/unet_i2vgen_ref.py's module, the epilogue's rounding is numpy's, and the entry points refuse what they
must before any launch."""
import ctypes

import numpy as np
import torch

import helpers  # noqa: F401
import helper_forms as HF
import shell_forms as S

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# the tables hold the declared edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    assert (S.THREADS, S.MAX_LAT, S.GROUP16, S.TAIL_W, S.TAIL_H, S.TAIL_CK, S.TC_FRAMES, S.TC_PV) == (256, 8, 16, 32, 8, 32, 4, 4)
    assert (S.JOIN_C, S.JOIN_P, S.JOIN_CPT, S.ENC_WTS) == (32, 64, 8, 288) and S.JOIN_C * S.JOIN_P == S.THREADS * S.JOIN_CPT
    assert [S.enc_P(F) for F in S.ENC_FS] == [256, 128, 85, 51, 36, 16, 8, 8]
    assert S.ENC_OFF["b2"] + 4 == S.ENC_WTS and S.TAIL_W * S.TAIL_H == S.THREADS


def test_join_table_holds_the_declared_edges():
    base = S.JOIN[:20]
    assert {(c.HW, c.C2, c.B, c.F) for c in base} == {(p, c, b, f) for p in (1, 63, 64, 65, 130) for c in (32, 96) for (b, f) in ((1, 1), (2, 3))}
    assert {p - S.JOIN_P for p in S.JOIN_HWS} >= {-1, 0, 1} and max(S.JOIN_HWS) > 2 * S.JOIN_P and min(S.JOIN_HWS) == 1
    assert {c // S.JOIN_C for c in S.JOIN_C2S} == {1, 3}
    assert {(c.res, c.res_dt) for c in S.JOIN} == {("none", F32)} | {(l, d) for l in ("4d", "5d") for d in S.DTYPES}
    assert {c.col for c in S.JOIN} == {0, 64} and {c.mirror for c in S.JOIN} == {"none", "plain", "split"}
    assert any(c.ld_skip > c.C2 and not c.inplace for c in S.JOIN)
    split = [c for c in S.JOIN if c.mirror == "split"]
    assert any(c.lo_off == c.col + c.C2 for c in split) and any(c.lo_off == c.col + c.C2 and c.col for c in split)
    far = [c for c in split if c.lo_off > c.col + c.C2]
    assert far and all(c.lo_off + c.col + c.C2 < 2 * c.ld_out for c in far)          # poison between hi and lo, and behind lo
    assert all(c.lo_off % 8 == 0 and c.lo_off + c.col + c.C2 <= 2 * c.ld_out for c in split) and all(c.lo_off == 0 for c in S.JOIN if c.mirror != "split")
    assert {c.mirror for c in S.JOIN if c.inplace} == {"plain", "split"} and all(c.col == 0 and c.ld_skip == c.ld_out and c.res != "none" for c in S.JOIN if c.inplace)
    assert any(c.B * c.F > 1 and c.res == "5d" for c in split) and any(c.B * c.F > 1 and c.res == "4d" for c in S.JOIN)
    for c in S.JOIN:
        v = S.join_values(c)
        assert float(v.abs().max()) < 65504.0 and float(v.abs().max()) > 2.0e4, c.id
        lo = (v - v.half().float()).half()
        assert bool(((lo != 0) & (lo.float().abs() < 2.0 ** -14)).any()), c.id          # fp16 subnormals among the lo halves
        if c.res != "none":          # the restated index arithmetic is the permutation the layouts declare
            skip, res = S.join_problem(c.id)
            r4 = res if c.res == "4d" else res.reshape(c.B, c.C2, c.F, c.HW).permute(0, 2, 1, 3).reshape(c.B * c.F, c.C2, c.HW)
            assert torch.equal(v, skip + r4.float().permute(0, 2, 1).reshape(-1, c.C2)), c.id
    assert len({c.id for c in S.JOIN}) == len(S.JOIN)


def test_posterior_table_holds_the_declared_edges():
    assert {c.N * c.hw - S.THREADS for c in S.POSTERIOR if c.N == 1} == {-1, 0, 1}
    assert any(c.N == 3 and c.hw < S.THREADS and S.THREADS % c.hw != 0 and c.N * c.hw > S.THREADS for c in S.POSTERIOR)          # a workgroup over two images
    assert max(S.PO_LATS) == S.MAX_LAT and min(S.PO_LATS) == 1
    for lat in S.PO_LATS:
        t = [c for c in S.POSTERIOR if c.lat == lat]
        assert {(c.N, c.hw) for c in t} == set(S.PO_SHAPES) and {c.kind for c in t} == {0, 1, 2} and {c.out_dt for c in t} == set(S.DTYPES)
        assert {c.eps_dt for c in t if c.kind == S.PSAMPLE} == set(S.DTYPES) and {c.wq for c in t} == set(S.PO_WQ)
        assert {c.nchw for c in t} == {0, 1} and {c.scale for c in t} == set(S.PO_SCALES)
        assert {(c.kind, c.out_dt) for c in t} == {(k, d) for k in (0, 1, 2) for d in S.DTYPES}
        assert {(c.kind, c.wq) for c in t} == {(k, q) for k in (0, 1, 2) for q in S.PO_WQ}
    saw_overflow = False
    for c in S.POSTERIOR:
        assert c.ldx == 2 * c.lat + (3 if c.nchw else 8)
        xbuf, wq, bq, eps = S.posterior_problem(c.id)
        assert int(torch.isnan(xbuf).sum()) == (c.ldx - 2 * c.lat) * c.N * c.hw
        assert (wq is None) == (c.wq == "none") and (bq is None) == (c.wq != "both")
        pre = S.posterior_prelogvar(c)
        for want in S.PO_LV:          # each planted value before the clamp, to what the solve leaves of it
            assert float((pre - want).abs().min()) < 1e-4, (c.id, want)
        assert float(pre.min()) < -30.0 and float(pre.max()) > 20.0
        ref, bound = S.posterior_reference(c)
        if c.out_dt == F16:          # nothing within its bound of the fp16 overflow threshold: the GPU test needs no exclusion list
            assert bool(((ref.abs() - S.FP16_OVF).abs() > bound).all()), c.id
            saw_overflow |= bool((ref.abs() >= S.FP16_OVF).any())
    assert saw_overflow          # exp(20) in an fp16 MOMENTS output
    assert len({c.id for c in S.POSTERIOR}) == len(S.POSTERIOR)


def test_head_and_tail_tables_hold_the_declared_edges():
    assert {(c.h, c.w, c.Cout, c.lat) for c in S.HEAD} == {(h, w, o, l) for (h, w) in ((1, 1), (1, 9), (9, 1), (5, 17), (13, 21)) for o in (16, 48, 128)
                                                         for l in (1, 4, 8)}
    assert {o // S.GROUP16 for o in S.HD_COUTS} == {1, 3, 8} and max(S.HD_LATS) == S.MAX_LAT
    for lat in S.HD_LATS:
        assert {c.dt for c in S.HEAD if c.lat == lat} == set(S.DTYPES) and {c.frames for c in S.HEAD if c.lat == lat} == {1, 3}
    n = [c.h * c.w * c.Cout // S.GROUP16 for c in S.HEAD]
    assert any(v > S.THREADS and v % S.THREADS for v in n) and any(v < S.THREADS for v in n)
    for c in S.HEAD:
        clip, wpq, bpq = S.head_problem(c.id)[:3]
        assert float(bpq.abs().min()) > 0.2 and int(torch.isnan(clip.float()).sum()) == (c.frames - 1) * c.lat * c.h * c.w
    # the tail
    assert {c.W for c in S.TAIL if c.H == 9} >= set(S.TL_WS) and {c.H for c in S.TAIL if c.W == 33} >= set(S.TL_HS)
    assert {w - S.TAIL_W for w in S.TL_WS} >= {-1, 0, 1} and max(S.TL_WS) > 2 * S.TAIL_W and min(S.TL_WS) == 1
    assert {h - S.TAIL_H for h in S.TL_HS} >= {-1, 0, 1} and max(S.TL_HS) > 2 * S.TAIL_H and min(S.TL_HS) == 1
    assert {c.C for c in S.TAIL} == {32, 64, 96, 160} and {c.C // 32 for c in S.TAIL} == {1, 2, 3, 5}
    assert {c.C // S.TAIL_CK for c in S.TAIL} == {1, 2, 3, 5} and S.TAIL_CK % 5 != 0 and S.TAIL_CK % 3 != 0          # groups straddle the chunks
    assert {c.Cout for c in S.TAIL if c.C == 96} == {1, 2, 3, 4} and {c.Cout for c in S.TAIL} == {1, 2, 3, 4}
    for c in S.TAIL:
        x, stats, gamma, beta, w, b = S.tail_problem(c.id)
        sc, sf, var0 = S.tail_scales(c, stats, gamma, beta)
        assert float((sf * torch.sigmoid(sf)).min()) > 0.3, c.id          # what a kernel that pads x, not the activated map, puts on the border
        ref, _ = S.tail_reference(c.id)
        assert c.H * c.W < 64 or (float(ref.min()) < -1.0 and float(ref.max()) > 1.0), c.id          # both clamp edges (a 9-pixel map may miss one)
        if c.flat is not None:
            cg = c.C // 32
            assert bool((var0[c.flat * cg:(c.flat + 1) * cg] < -S.TL_EPS).all())          # the clamp decides: var + eps would be negative
            assert bool(torch.isfinite(S.tail_emulate(c.id)).all())
    flat, tie = S.pick(S.TAIL, flat=5), S.pick(S.TAIL, tie=126)
    s32 = S.tail_emulate(tie.id)
    u = s32[:, 0] * 0.5 + 0.5
    assert bool((s32[:, 0] == S.tie_bias(126)).all()) and bool((u * 255.0 == 126.5).all())          # an exact tie on an even integer
    assert bool((S.epilogue(s32, S.BYTES, F32)[..., 0] == 126).all()) and bool((S.epilogue(s32, S.BYTES, F32, "half_away")[..., 0] == 127).all())
    assert flat.C == 96 and len({c.id for c in S.TAIL}) == len(S.TAIL) and len({c.id for c in S.HEAD}) == len(S.HEAD)


def test_time_conv_table_holds_the_declared_edges():
    assert {(c.OC, c.F, c.HW) for c in S.TIME_CONV} == {(o, f, p) for o in (1, 2, 3, 4) for f in (1, 3, 4, 5, 8, 9) for p in (4, 1020, 1024, 1028, 1, 255, 257, 1026)}
    assert {f - S.TC_FRAMES for f in S.TC_FS} >= {-1, 0, 1} and 2 * S.TC_FRAMES in S.TC_FS and 2 * S.TC_FRAMES + 1 in S.TC_FS and 1 in S.TC_FS
    assert all(p % S.TC_PV == 0 for p in S.TC_HW_VEC) and {p // S.TC_PV - S.THREADS for p in S.TC_HW_VEC} >= {-1, 0, 1} and min(S.TC_HW_VEC) == S.TC_PV
    assert all(p % S.TC_PV for p in S.TC_HW_SCALAR) and {p - S.THREADS for p in S.TC_HW_SCALAR} >= {-1, 1} and max(S.TC_HW_SCALAR) > 4 * S.THREADS
    assert len(S.TC_KINDS) == 9 and all(S.TC_BY_ID[i].OC == 3 and S.TC_BY_ID[i].F == 5 for i in S.TC_KIND_CASES)
    assert {S.TC_BY_ID[i].vec for i in S.TC_KIND_CASES} == {True, False} and all(S.TC_BY_ID[i].vec for i in S.TC_MISALIGN_CASES)
    assert any(S.TC_BY_ID[i].HW // S.TC_PV > S.THREADS for i in S.TC_MISALIGN_CASES)
    names = {m[0] for m in S.TC_MISALIGN}
    assert names == {"x + 4", "f32 out + 4", "unit out + 4", "f16 out + 4", "bf16 out + 4", "u8 out + 1", "u8 out + 2"}
    for name, xo, kind, dt, oo in S.TC_MISALIGN:          # each breaks exactly the rule it names: 16 (x, fp32), 8 (fp16 / bf16), 4 (bytes)
        rule = 4 if kind == S.BYTES else (16 if (kind == S.UNIT or dt == F32) else 8)
        assert (xo % 16 != 0) != (oo % rule != 0), name
        assert oo == 0 or oo % {S.BYTES: 1}.get(kind, 4 if (kind == S.UNIT or dt == F32) else 2) == 0          # still a whole element
    x, w, b, ref, _ = S.time_conv_problem(S.TC_KIND_CASES[0])
    assert float(ref.min()) < -1.0 and float(ref.max()) > 1.0


def test_encoder_pool_and_text_time_tables_hold_the_declared_edges():
    assert {c.F for c in S.ENCODER} == {1, 2, 3, 5, 7, 16, 31, 32}
    for F in S.ENC_FS:
        t, P = [c for c in S.ENCODER if c.F == F], S.THREADS // F
        assert {c.npix for c in t} == {P - 1, P, P + 1, 2 * P + 1} and all(c.P == P and c.B * c.HW == c.npix for c in t)
        assert all((c.B == 2) == (c.npix % 2 == 0) for c in t) and any(c.B == 2 and c.HW < P for c in t)          # a workgroup over both clips
        assert {c.dt for c in t} == (set(S.DTYPES) if F in (3, 32) else {F32}) and {c.kind for c in t} == set(S.ENC_KINDS)
    assert {F for F in S.ENC_FS if F * (S.THREADS // F) < S.THREADS} == {3, 5, 7, 31}          # idle lanes, f * P + pl no plain reshape
    for c in S.ENCODER:
        ref, bound, spread, top = S.enc_reference(c.id)[:4]
        if c.kind == "saturated" and c.F > 1:
            assert float((spread > 40.0).float().mean()) > 0.8 and float((top > 1.0 - 1e-6).float().mean()) > 0.5, c.id
        if c.kind == "equal":
            assert float((top - 1.0 / c.F).abs().max()) < 1e-12, c.id
    # the pooling
    assert {(c.x_dt, c.y_dt) for c in S.AAPOOL if c.N == 1} == {(a, b) for a in (F32, F16) for b in (F32, F16)}
    assert {(c.H, c.W, c.OH, c.OW) for c in S.AAPOOL} >= {(5, 7, 32, 32), (33, 47, 8, 16), (32, 32, 32, 32)} and any(c.OH != c.OW for c in S.AAPOOL)
    n2 = [c.N * c.OH * c.OW * c.C for c in S.AAPOOL if c.N == 2]
    assert any(n % S.THREADS and n < S.THREADS for n in n2) and any(n % S.THREADS and n > S.THREADS for n in n2)
    assert all(bool(S.aap_problem(c)[3].all()) for c in S.AAPOOL if (c.H, c.W) == (c.OH, c.OW))
    assert any(bool(S.aap_problem(c)[3].any()) and not bool(S.aap_problem(c)[3].all()) for c in S.AAPOOL)          # replication beside two-element windows
    # text_time
    assert {(c.text_dim, c.dim, c.n_ids, c.B) for c in S.TEXT_TIME} == {(t, d, n, b) for t in (1, 255, 256, 257, 1280) for d in (2, 6, 256) for n in (1, 6)
                                                                     for b in (1, 3)}
    assert {t - S.THREADS for t in S.TT_TEXT} >= {-1, 0, 1} and max(S.TT_TEXT) > 4 * S.THREADS and {c.dt for c in S.TEXT_TIME} == set(S.DTYPES)
    assert max(n * d // 2 for n in S.TT_IDS for d in S.TT_DIMS) > 2 * S.THREADS and S.TT_PAD > 0
    assert {float(v) for c in S.TEXT_TIME for v in S.tt_problem(c)[1].reshape(-1)} == set(HF.SC_TS)
    assert (HF.SC_C, HF.SC_K) == (2.0, 4.0)
    for tab in (S.ENCODER, S.AAPOOL, S.TEXT_TIME, S.TIME_CONV):
        assert len({c.id for c in tab}) == len(tab)


# ---------------------------------------------------------------------------------------------------------------------------
# the emulations stay within their bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _with(name, value, fn):
    old = getattr(S, name)
    setattr(S, name, value)
    S.enc_reference.cache_clear()
    try:
        return fn()
    finally:
        setattr(S, name, old)
        S.enc_reference.cache_clear()


def _po_share():
    """std and var of every case (MOMENTS in fp32, whatever the case stores) against their own bounds"""
    w = 0.0
    for c in S.POSTERIOR:
        (_, _, std, var), (_, _, dstd, dvar) = S.posterior_moments64(c)
        em = S.posterior_emulate(c, kind=S.MOMENTS, out_dt=F32).double()
        w = max(w, S.check(em[:, 2 * c.lat:3 * c.lat], S._po_layout(c, [std]), S._po_layout(c, [dstd])),
                S.check(em[:, 3 * c.lat:], S._po_layout(c, [var]), S._po_layout(c, [dvar])))
    return w


def _enc_share():
    return max(max(S.enc_stage_shares(c.id)) for c in S.ENCODER)


def test_emulations_stay_within_their_bounds():
    for name, fn, note in (("PO_E", _po_share, "vae_posterior, std and var"), ("EN_K", _enc_share, "i2v_latent_encoder, the worst of its three stages")):
        k = getattr(S, name)
        share, lower = fn(), _with(name, k / 2, fn)
        print("SHELL-HOST %-4s = 2^%-3d share %.3f   one power of two lower: %.3f   (%s)" % (name, round(torch.log2(torch.tensor(k)).item()), share, lower, note))
        assert share <= 0.5 < lower, (name, share, lower)
    st = [max(S.enc_stage_shares(c.id)[i] for c in S.ENCODER) for i in range(3)]
    print("SHELL-HOST encoder stages: LayerNorm %.3f  softmax weights %.3f  erf GELU %.3f" % tuple(st))
    worst = {}

    def take(fam, v):
        worst[fam] = max(worst.get(fam, 0.0), v)

    for c in S.POSTERIOR:
        take("vae_posterior", S.overflow_check(S.posterior_emulate(c), *S.posterior_reference(c), c.out_dt))
    for c in S.HEAD:
        take("vae_dec_head", S.check(S.head_emulate(c.id), *S.head_problem(c.id)[5:7]))
    for c in S.TAIL:
        take("vae_dec_tail", S.check(S.tail_emulate(c.id), *S.tail_reference(c.id)))
    for c in S.TIME_CONV:
        if c.HW <= 257 or c.OC == 3:
            take("vae_time_conv", S.check(S.time_conv_emulate(c.id), *S.time_conv_problem(c.id)[3:5]))
    for c in S.ENCODER:
        take("i2v_latent_encoder", S.check(S.enc_emulate(c.id), *S.enc_reference(c.id)[:2]))
    for c in S.AAPOOL:
        x, ref, bound, one = S.aap_problem(c)
        out = S.aap_emulate(c)
        take("adaptive_avgpool", S.check(out, ref, bound))
        xi = x[:, [a for a, _ in S.aap_windows(c.H, c.OH)]][:, :, [a for a, _ in S.aap_windows(c.W, c.OW)]]
        assert torch.equal(out[one], xi.float().to(c.y_dt)[one]), c.id          # a one-element window is a conversion
    for c in S.TEXT_TIME:
        take("unet_text_time", S.check(S.tt_emulate(c), *S.tt_problem(c)[2:4]))
    for fam, v in sorted(worst.items()):
        print("SHELL-HOST %-20s worst emulation / bound %.3f" % (fam, v))
        assert v <= 1.0, (fam, v)
    assert worst["unet_text_time"] <= 0.5          # helper_forms' SC_C and SC_K, calibrated there, hold their half here as well


# ---------------------------------------------------------------------------------------------------------------------------
# every planted error is rejected on a named case
# ---------------------------------------------------------------------------------------------------------------------------
def test_planted_errors_are_rejected():
    # posterior
    po = lambda **kw: S.pick(S.POSTERIOR, **kw)
    for c, planted in ((po(kind=S.MOMENTS, out_dt=F32, lat=4), "clamp30"), (po(kind=S.MOMENTS, out_dt=F32, lat=8), "std_explv"),
                       (po(kind=S.PSAMPLE, lat=3, out_dt=F32), "std_explv"), (po(kind=S.MODE, wq="both", lat=1), "no_bq"), (po(kind=S.MOMENTS, wq="both", lat=8), "no_bq"),
                       (po(nchw=1, N=3, lat=4), "nchw_stride"), (po(nchw=1, N=3, lat=1), "nchw_stride"), (po(kind=S.PSAMPLE, scale=0.18215, lat=4), "noise_unscaled"),
                       (po(kind=S.PSAMPLE, scale=0.18215, lat=8, out_dt=BF16), "noise_unscaled")):
        ref, bound = S.posterior_reference(c)
        assert S.overflow_check(S.posterior_emulate(c), ref, bound, c.out_dt) <= 1.0, c.id
        assert S.overflow_check(S.posterior_emulate(c, planted), ref, bound, c.out_dt) > 1.0, (c.id, planted)
    # head: a border pixel that saw bpq outside the map (even on 1 x 1), the scale in the wrong place, a clip frame read densely
    for cid, planted in (("hd-1x1-Co16-lat1-f32-dense", "bpq_outside"), (S.pick(S.HEAD, h=13, w=21, Cout=48, lat=4).id, "bpq_outside"),
                         (S.pick(S.HEAD, h=5, w=17, lat=8).id, "scale_after"), (S.pick(S.HEAD, h=9, w=1, lat=1).id, "scale_after"),
                         (S.pick(S.HEAD, frames=3, lat=4).id, "clip_stride"), (S.pick(S.HEAD, frames=3, lat=8, h=13).id, "clip_stride")):
        assert cid in S.HD_BY_ID
        ref, bound = S.head_problem(cid)[5:7]
        assert S.check(S.head_emulate(cid, planted), ref, bound) > 1.0, (cid, planted)
    c = S.pick(S.HEAD, h=13, w=21, Cout=48, lat=4)          # ... and only the border is hit: what a rel-inf bound would have to see
    ref, bound = S.head_problem(c.id)[5:7]
    bad = ((S.head_emulate(c.id, "bpq_outside").double() - ref).abs() > bound).reshape(c.h, c.w, c.Cout).any(-1)
    assert bool(bad[0].all()) and bool(bad[:, 0].all()) and not bool(bad[1:-1, 1:-1].any())
    # tail
    for cid, planted in (("tl-9x33-C96-Co3-all", "pad_before_act"), ("tl-9x1-C32-Co1", "pad_before_act"), ("tl-9x31-C64-Co2", "first_chunk_scales"),
                         ("tl-9x33-C160-Co4", "first_chunk_scales"), ("tl-9x32-C96-Co3", "group_c32"), ("tl-8x33-C160-Co1", "group_c32"),
                         ("tl-9x33-C96-Co2-all", "no_halo_x32"), ("tl-9x65-C32-Co2", "no_halo_x32"), ("tl-9x33-C96-Co3-flat", "unclamped")):
        assert S.check(S.tail_emulate(cid, planted), *S.tail_reference(cid)) > 1.0, (cid, planted)
    s32 = S.tail_emulate("tl-7x33-C32-Co2-tie")
    assert not S.bits_equal(S.epilogue(s32, S.BYTES, F32), S.epilogue(s32, S.BYTES, F32, "half_away"))
    s32 = S.tail_emulate("tl-9x33-C96-Co3-all")
    assert not S.bits_equal(S.epilogue(s32, S.UNIT, F16), S.epilogue(s32, S.UNIT, F16, "unit_unrounded"))
    assert S.bits_equal(S.epilogue(s32, S.UNIT, F32), S.epilogue(s32, S.UNIT, F32, "unit_unrounded"))
    # time conv
    for cid, planted in (("tc-OC3-F5-HW257", "seam_zero"), ("tc-OC1-F8-HW4", "seam_zero"), ("tc-OC2-F3-HW255", "taps_reversed"),
                         ("tc-OC1-F9-HW1", "taps_reversed"), ("tc-OC4-F4-HW4", "w_transposed"), ("tc-OC2-F1-HW1", "w_transposed")):
        ref, bound = S.time_conv_problem(cid)[3:5]
        assert S.check(S.time_conv_emulate(cid), ref, bound) <= 1.0 and S.check(S.time_conv_emulate(cid, planted), ref, bound) > 1.0, (cid, planted)
    c = S.TC_BY_ID["tc-OC3-F5-HW257"]          # the seam error sits on the frames f = 3 | 4 alone
    ref, bound = S.time_conv_problem(c.id)[3:5]
    bad = ((S.time_conv_emulate(c.id, "seam_zero").double() - ref).abs() > bound).any(2).any(1)
    assert bad.tolist() == [False, False, False, True, True]
    s32 = S.time_conv_emulate("tc-OC3-F5-HW1028")
    assert not S.bits_equal(S.epilogue(s32, S.BYTES, F32), S.epilogue(s32, S.BYTES, F32, "bytes_reversed"))
    # join
    sp = S.pick(S.JOIN, mirror="split", B=2, res="5d", inplace=False)
    v = S.join_values(sp)
    for planted in ("lo_zero", "lo_shifted"):
        assert not S.bits_equal(S.join_mirror(sp, v), S.join_mirror(sp, v, planted)), planted
    tight = S.pick(S.JOIN, mirror="split", lo_off=32, col=0)
    assert not S.bits_equal(S.join_mirror(tight, S.join_values(tight)), S.join_mirror(tight, S.join_values(tight), "lo_shifted"))
    for c in (S.pick(S.JOIN, res="4d", B=2), S.pick(S.JOIN, res="5d", B=2)):
        for planted in ("layout_swapped", "bf_swapped"):
            assert not S.bits_equal(S.join_values(c), S.join_values(c, planted)), (c.id, planted)
    # encoder
    for cid, planted in ((S.pick(S.ENCODER, F=3, kind="plain", dt=F32).id, "scale_one"), (S.pick(S.ENCODER, F=3, kind="plain", dt=F32).id, "extra_key"),
                         (S.pick(S.ENCODER, F=7, kind="plain").id, "extra_key"), (S.pick(S.ENCODER, F=3, kind="plain", dt=F32).id, "stride_up"),
                         (S.pick(S.ENCODER, F=31, kind="plain").id, "stride_up"), (S.pick(S.ENCODER, F=1, kind="plain").id, "tanh_gelu"),
                         (S.pick(S.ENCODER, F=16, kind="plain").id, "heads_swapped"), (S.pick(S.ENCODER, F=32, kind="saturated", dt=F32).id, "scale_one")):
        ref, bound = S.enc_reference(cid)[:2]
        assert S.check(S.enc_emulate(cid), ref, bound) <= 1.0 and S.check(S.enc_emulate(cid, planted), ref, bound) > 1.0, (cid, planted)
    # pooling, text_time
    c = S.pick(S.AAPOOL, H=33, OH=8, x_dt=F32, y_dt=F32)
    assert S.check(S.aap_emulate(c, "floor_end"), *S.aap_problem(c)[1:3]) > 1.0
    for c, planted in ((S.pick(S.TEXT_TIME, dim=2, n_ids=1, B=3), "sin_cos"), (S.pick(S.TEXT_TIME, dim=256, n_ids=6), "sin_cos"),
                       (S.pick(S.TEXT_TIME, dim=6, n_ids=6, B=3), "full_dim"), (S.pick(S.TEXT_TIME, dim=256, n_ids=1, B=3), "full_dim")):
        assert S.check(S.tt_emulate(c, planted), *S.tt_problem(c)[2:4]) > 1.0, (c.id, planted)


# ---------------------------------------------------------------------------------------------------------------------------
# restatements against independent formulations
# ---------------------------------------------------------------------------------------------------------------------------
def test_encoder_reference_is_the_restated_module():
    """the forms' fp64 chain (whose intermediates carry the bound) equals unet_i2vgen_ref.LatentTemporalEncoderRef with the same 288 weights"""
    import unet_i2vgen_ref as R
    for sat in (False, True):
        enc = R.LatentTemporalEncoderRef(4, 2, 4, 16).double().eval()
        enc.load_state_dict({k: v.double() for k, v in S.enc_state_dict(S.enc_weights(sat)).items()})
        for c in S.ENCODER:
            if (c.kind == "saturated") != sat or c.dt != F32:
                continue
            x = S.enc_problem(c.id)[0]
            with torch.no_grad():
                want = S.enc_rows(c, enc(S.enc_tokens(c, x.double())))
            ref = S.enc_reference(c.id)[0]
            assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max()), c.id


def test_epilogue_is_numpys_rounding_and_the_older_tests_restatement():
    g = torch.Generator().manual_seed(11)
    s32 = torch.randn(2, 3, 5, 7, generator=g) * 1.5
    s32.view(-1)[:4] = torch.tensor([S.tie_bias(126), S.tie_bias(200), -1.0, 1.0])
    for dt in S.DTYPES:
        s = s32.to(dt)
        unit = (s.float() / 2 + 0.5).clamp(0, 1)
        assert torch.equal(S.epilogue(s32, S.SAMPLE, dt), s) and torch.equal(S.epilogue(s32, S.UNIT, dt), unit)
        want = (unit.permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
        assert np.array_equal(S.epilogue(s32, S.BYTES, dt).numpy(), want)
    b = S.epilogue(s32, S.BYTES, F32).reshape(-1)
    assert int(b[0]) == 126 and int(b[3]) == 200 and {0, 255} <= {int(v) for v in b}


# ---------------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    rows = S.refusals(0x10000, 0x10004)
    assert len({r[0] for r in rows}) == len(rows) >= 36
    named = {r[0] for r in rows}
    assert {"join lo_off % 8", "join lo_off < col + C2", "join lo beyond the row", "join lo_off without a mirror", "join misaligned skip", "join C2 = 48"} <= named
    for name, sym, args, msg in rows:
        rc = getattr(lib, sym)(*args, ctypes.c_void_p(0))
        err = (lib.ctrl_last_error() or b"").decode()
        assert rc != 0 and msg in err, (name, rc, err)
