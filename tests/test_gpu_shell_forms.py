"""The per-pixel shell kernels around the KL-VAE and the backbone UNets (vae_posterior, vae_dec_head, vae_dec_tail, vae_time_conv of
csrc/vae.hip; unet_skip_join, i2v_latent_encoder, adaptive_avgpool_nhwc, unet_text_time of csrc/unet.hip) on the GPU: every case of
tests/shell_forms.py through the C entry points, against the exact restatements bit for bit or against the fp64 references and their
element-wise bounds.  Every output lies inside a poisoned allocation (helpers.Guarded), so a strided, partial or misaligned result also
proves that nothing outside it was written; inputs are surrounded by NaN.  The checks themselves are tested on the host
(tests/test_shell_check_host.py).  Nothing here provokes a fault: every refused call returns before a launch.  One PARITY line per kernel
gives the worst share of its bound.

Measured on the MI355X (worst |err| / bound over the kernel's cases; the fp32 CPU emulation's figure in brackets):
    unet_skip_join          41 checks bit-exact (23 masters, 17 mirror rows with their poison, lo_off = 0 through the split entry)
    vae_posterior           72 cases  0.598 (0.500); 128 fp16 MOMENTS results beyond 65520 came back as +inf
    vae_dec_head            45 cases  0.172 (0.172)
    vae_dec_tail            15 cases  0.009 (0.009), 120 epilogue results bit-exact
    vae_time_conv          192 cases  0.472 (0.394 on the emulated subset), 16 epilogue and 28 misaligned results bit-exact
    i2v_latent_encoder      48 cases  0.004 (0.004), 144 copies bit-exact
    adaptive_avgpool_nhwc   18 cases  0.500 (0.500: the fp16 store), 8 sets of one-element windows bit-exact
    unet_text_time          60 cases  0.269 (0.271), the text columns bit-exact
"""
import ctypes as C

import pytest
import torch

import helpers
import shell_forms as S
from helpers import Guarded
from test_gpu_helper_forms import Worst, _inp, _out, _untouched

pytestmark = pytest.mark.gpu
F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8
U8_POISON = 77


@pytest.fixture(scope="module")
def L_(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def ops(L_):
    from ctrl_adapter_amd import ops
    return ops


def _out1d(n, dt, dev, byte_off=0):
    """n elements of dt inside poison, the first one `byte_off` bytes behind a 16-byte boundary"""
    es = torch.empty(0, dtype=dt).element_size()
    assert byte_off % es == 0
    start = 64 // es + byte_off // es
    full = start + n + 64 // es
    if dt == U8:
        g = Guarded((full,), (slice(start, start + n),), U8, dev, U8_POISON)
        g._snap = helpers._bits(g.buf).clone()
    else:
        g = Guarded.out((full,), (slice(start, start + n),), dt, dev)
    assert g.view.data_ptr() % 16 == byte_off % 16
    return g


def _kind_dt(kind, dt):
    """the element type an epilogue kind stores"""
    return {S.SAMPLE: dt, S.UNIT: F32, S.BYTES: U8}[kind]


# ---------------------------------------------------------------------------------------------------------------------------
# unet_skip_join
# ---------------------------------------------------------------------------------------------------------------------------
def _join(L_, dev, c):
    skip, res = S.join_problem(c.id)
    rows = skip.shape[0]
    g32 = Guarded.out((rows + 2, c.ld_out), (slice(1, rows + 1), slice(c.col, c.col + c.C2)), F32, dev)
    if c.inplace:
        g32.view.copy_(skip)
        gs, sp = None, g32.buf[1:]
    else:
        gs = _inp(skip, dev, c.ld_skip - c.C2)
        sp = gs.view
    gr = _inp(res.reshape(-1), dev) if res is not None else None
    g16 = None
    if c.mirror != "none":
        ld16 = c.ld_out * (2 if c.mirror == "split" else 1)
        end = c.col + c.C2 + (c.lo_off if c.mirror == "split" else 0)
        g16 = Guarded.out((rows + 2, ld16), (slice(1, rows + 1), slice(c.col, end)), F16, dev)
    args = [L_.ptr(sp), c.ld_skip, L_.ptr(gr.view) if gr else None, L_.dtype_code(c.res_dt), int(c.res == "5d"), c.B, c.F, c.HW, c.C2,
            L_.ptr(g32.buf[1:]), L_.ptr(g16.buf[1:]) if g16 else None, c.ld_out, c.col]
    if c.mirror == "split":
        L_.check(L_.lib().ctrl_op_unet_skip_join_split(*args, c.lo_off, L_.cur_stream()))
    else:
        L_.check(L_.lib().ctrl_op_unet_skip_join(*args, L_.cur_stream()))
    _untouched(c.id, gs, gr, g32, g16)
    return g32, g16


def test_skip_join_with_plain_and_split_mirrors(L_, gpu):
    """one fp32 add, hi = fp16(v), lo = fp16(v - hi): bit for bit, the mirror rows compared WITH their poison (the columns between hi and lo
    and behind lo); a plain mirror through the split entry with lo_off = 0 gives the old entry's bits"""
    w = Worst("unet_skip_join")
    for c in S.JOIN:
        v = S.join_values(c)
        g32, g16 = _join(L_, gpu, c)
        w.exact(c.id + " master", g32.view, v)
        if g16 is not None:
            w.exact(c.id + " mirror", g16.buf[1:-1], S.join_mirror(c, v))
    c = S.pick(S.JOIN, mirror="plain", inplace=False)
    skip, res = S.join_problem(c.id)
    rows = skip.shape[0]
    g32, g16 = _out((rows, c.ld_out), F32, gpu), _out((rows, c.ld_out), F16, gpu)
    sd, rd = skip.to(gpu), (res.to(gpu) if res is not None else None)
    L_.check(L_.lib().ctrl_op_unet_skip_join_split(L_.ptr(sd), c.C2, L_.ptr(rd), L_.dtype_code(c.res_dt),
                                                   int(c.res == "5d"), c.B, c.F, c.HW, c.C2, L_.ptr(g32.view), L_.ptr(g16.view), c.ld_out, c.col, 0,
                                                   L_.cur_stream()))
    _untouched(c.id, g32, g16)
    w.exact(c.id + " lo_off 0", g16.view[:, c.col:c.col + c.C2].contiguous(), S.join_values(c).half())
    w.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# vae_posterior
# ---------------------------------------------------------------------------------------------------------------------------
def test_vae_posterior(L_, gpu):
    """every element under its bound (the clamp is continuous: none is exempt); an fp16 result whose reference lies beyond 65520 must be that
    infinity (exp(20) in MOMENTS)"""
    w = Worst("vae_posterior")
    infs = 0
    for c in S.POSTERIOR:
        xbuf, wq, bq, eps = S.posterior_problem(c.id)
        ref, bound = S.posterior_reference(c)
        gx, ge = _inp(xbuf, gpu), _inp(eps, gpu)
        gw, gb = (_inp(wq, gpu) if wq is not None else None), (_inp(bq, gpu) if bq is not None else None)
        go = _out((ref.numel(),), c.out_dt, gpu)
        L_.check(L_.lib().ctrl_op_vae_posterior(L_.ptr(gx.view), c.ldx, c.nchw, L_.ptr(gw.view) if gw else None, L_.ptr(gb.view) if gb else None, c.N, c.lat,
                                                1, c.hw, L_.ptr(ge.view) if c.kind == S.PSAMPLE else None, L_.dtype_code(c.eps_dt), c.scale, c.kind,
                                                L_.ptr(go.view), L_.dtype_code(c.out_dt), L_.cur_stream()))
        _untouched(c.id, gx, ge, gw, gb, go)
        out = go.view.cpu().reshape(ref.shape)
        ovf = (ref.abs() >= S.FP16_OVF) if c.out_dt == F16 else torch.zeros_like(ref, dtype=torch.bool)
        if bool(ovf.any()):
            infs += int(ovf.sum())
            assert bool((out[ovf].double() == torch.sign(ref[ovf]) * float("inf")).all()), "%s: an overflowing fp16 result must be that infinity" % c.id
        w.close(c.id, out[~ovf], ref[~ovf], bound[~ovf])
    print("vae_posterior: %d fp16 results beyond 65520 came back as their infinity" % infs)
    assert infs > 0
    w.done()


# ---------------------------------------------------------------------------------------------------------------------------
# vae_dec_head, vae_dec_tail
# ---------------------------------------------------------------------------------------------------------------------------
def test_vae_dec_head(L_, ops, gpu):
    """dense latents and the middle frame of a clip whose other frames are NaN; element-wise, so a border pixel that saw bpq outside the map
    (the zero padding applies to the post_quant_conv RESULT) shows"""
    w = Worst("vae_dec_head")
    for c in S.HEAD:
        clip, wpq, bpq, wt, b, ref, bound = S.head_problem(c.id)
        gz, gq, gbq, gb = _inp(clip.reshape(-1), gpu), _inp(wpq, gpu), _inp(bpq, gpu), _inp(b, gpu)
        wd = ops.pack_conv_w_direct(wt.to(gpu))
        go = _out((c.h * c.w * c.Cout,), F32, gpu)
        hw = c.h * c.w
        z = C.c_void_p(gz.view.data_ptr() + (c.frames // 2) * hw * clip.element_size())
        L_.check(L_.lib().ctrl_op_vae_dec_head(z, L_.dtype_code(c.dt), c.scale, L_.ptr(gq.view), L_.ptr(gbq.view), L_.ptr(wd), L_.ptr(gb.view),
                                               L_.ptr(go.view), c.lat, c.h, c.w, c.frames * hw, c.Cout, L_.cur_stream()))
        _untouched(c.id, gz, gq, gbq, gb, go)
        w.close(c.id, go.view.reshape(ref.shape), ref, bound)
    w.done()


def _tail(L_, dev, c, dev_in, kind, dt):
    gx, gs, gg, gbe, wd, gb = dev_in
    n = c.H * c.W * c.Cout
    go = _out1d(n, _kind_dt(kind, dt), dev)
    L_.check(L_.lib().ctrl_op_vae_dec_tail(L_.ptr(gx.view), L_.ptr(gs.view), L_.ptr(gg.view), L_.ptr(gbe.view), S.TL_EPS, L_.ptr(wd), L_.ptr(gb.view),
                                           c.H, c.W, c.C, c.Cout, kind, L_.ptr(go.view), L_.dtype_code(dt), L_.cur_stream()))
    _untouched(c.id, gx, gs, gg, gbe, gb, go)
    out = go.view.cpu()
    return out.reshape(1, c.H, c.W, c.Cout) if kind == S.BYTES else out.reshape(1, c.Cout, c.H, c.W)


def test_vae_dec_tail(L_, ops, gpu):
    """the statistics are given (fp32 roundings of the fp64 group sums: no other kernel in the loop).  The fp32 SAMPLE against fp64; every
    other kind and dtype bit for bit from the kernel's own fp32 SAMPLE (one rounding, / 2 + 0.5 clamped, x 255 half to even, NHWC bytes)"""
    w, we = Worst("vae_dec_tail"), Worst("vae_dec_tail epilogue")
    for c in S.TAIL:
        x, stats, gamma, beta, wt, b = S.tail_problem(c.id)
        ref, bound = S.tail_reference(c.id)
        dev_in = (_inp(x, gpu), _inp(stats, gpu), _inp(gamma, gpu), _inp(beta, gpu), ops.pack_conv_w_direct(wt.to(gpu)), _inp(b, gpu))
        s32 = _tail(L_, gpu, c, dev_in, S.SAMPLE, F32)
        w.close(c.id, s32, ref, bound)
        for kind in (S.SAMPLE, S.UNIT, S.BYTES):
            for dt in S.DTYPES:
                if (kind, dt) != (S.SAMPLE, F32):
                    we.exact("%s kind %d %s" % (c.id, kind, S.DT_NAME[dt]), _tail(L_, gpu, c, dev_in, kind, dt), S.epilogue(s32, kind, dt))
        if c.tie is not None:          # the exact ties u * 255 = 126.5 round to the even byte
            assert bool((s32[:, 0] == S.tie_bias(c.tie)).all()) and bool((_tail(L_, gpu, c, dev_in, S.BYTES, F32)[..., 0] == c.tie).all())
    w.done()
    we.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# vae_time_conv
# ---------------------------------------------------------------------------------------------------------------------------
def _time_conv(L_, dev, c, gx, gw, gb, kind, dt, out_off=0):
    n = c.F * c.OC * c.HW
    go = _out1d(n, _kind_dt(kind, dt), dev, out_off)
    L_.check(L_.lib().ctrl_op_vae_time_conv(L_.ptr(gx.view), L_.ptr(gw.view), L_.ptr(gb.view), c.F, 1, c.HW, c.OC, kind, L_.ptr(go.view),
                                            L_.dtype_code(dt), L_.cur_stream()))
    _untouched(c.id, gx, gw, gb, go)
    out = go.view.cpu()
    return out.reshape(c.F, c.HW, c.OC) if kind == S.BYTES else out.reshape(c.F, c.OC, c.HW)


def test_vae_time_conv(L_, gpu):
    """every template, frame counts around the frame group, the vector path across the 256-thread boundary and the scalar path: the fp32
    SAMPLE against fp64; the three kinds x three dtypes bit for bit from it on both paths"""
    w, we = Worst("vae_time_conv"), Worst("vae_time_conv epilogue")
    for c in S.TIME_CONV:
        x, wt, b, ref, bound = S.time_conv_problem(c.id)
        gx, gw, gb = _inp(x.reshape(-1), gpu), _inp(wt.reshape(-1), gpu), _inp(b, gpu)
        s32 = _time_conv(L_, gpu, c, gx, gw, gb, S.SAMPLE, F32)
        w.close(c.id, s32, ref, bound)
        if c.id in S.TC_KIND_CASES:
            for kind, dt in S.TC_KINDS:
                if (kind, dt) != (S.SAMPLE, F32):
                    we.exact("%s kind %d %s" % (c.id, kind, S.DT_NAME[dt]), _time_conv(L_, gpu, c, gx, gw, gb, kind, dt), S.epilogue(s32, kind, dt))
    w.done()
    we.done(True)


def test_vae_time_conv_scalar_path_gives_the_vector_paths_bits(L_, gpu):
    """vector-shaped data sent down the scalar kernel by each alignment rule in turn: x 4 bytes off, an fp32 / UNIT output 4 bytes off, an
    fp16 / bf16 output 4 bytes off (their rule is 8), bytes 1 and 2 off (their rule is 4): the same bits, nothing written outside"""
    we = Worst("vae_time_conv misaligned")
    for cid in S.TC_MISALIGN_CASES:
        c = S.TC_BY_ID[cid]
        x, wt, b, _, _ = S.time_conv_problem(cid)
        gw, gb = _inp(wt.reshape(-1), gpu), _inp(b, gpu)
        aligned = _inp(x.reshape(-1), gpu)
        for name, x_off, kind, dt, out_off in S.TC_MISALIGN:
            gx = Guarded.inp(x.reshape(-1), (8 + x_off // 4,), (8,), gpu)
            assert gx.view.data_ptr() % 16 == x_off and aligned.view.data_ptr() % 16 == 0
            want = _time_conv(L_, gpu, c, aligned, gw, gb, kind, dt)
            we.exact("%s %s" % (cid, name), _time_conv(L_, gpu, c, gx, gw, gb, kind, dt, out_off), want)
    we.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# i2v_latent_encoder
# ---------------------------------------------------------------------------------------------------------------------------
def test_i2v_latent_encoder(L_, gpu):
    """frame counts that leave idle lanes (P = 256 / F pixels per workgroup, slots f * P + pl), pixel counts around P, workgroups over both
    clips, a saturated and an exactly uniform softmax: columns 4..7 element-wise against the fp64 restatement; columns 0..3, keep and the
    precomputed pass bit for bit"""
    w, we = Worst("i2v_latent_encoder"), Worst("i2v_latent_encoder copies")
    for c in S.ENCODER:
        x, wts, sample = S.enc_problem(c.id)
        ref, bound = S.enc_reference(c.id)[:2]
        rows = x.shape[0]
        gx, gw, gs = _inp(x, gpu), _inp(wts, gpu), _inp(sample, gpu)
        go, gk = _out((rows, 8), F32, gpu), _out((rows, 4), F32, gpu)
        L_.check(L_.lib().ctrl_op_i2v_latent_encoder(L_.ptr(gx.view), L_.ptr(gw.view), L_.ptr(gs.view), L_.dtype_code(c.dt), L_.ptr(go.view), L_.ptr(gk.view),
                                                     c.B, c.F, c.HW, 0, L_.cur_stream()))
        _untouched(c.id, gx, gw, gs, go, gk)
        out = go.view.cpu()
        w.close(c.id, out[:, 4:], ref, bound)
        we.exact(c.id + " sample", out[:, :4].contiguous(), S.enc_sample_rows(c, sample))
        we.exact(c.id + " keep", gk.view, out[:, 4:].contiguous())
        g2 = _out((rows, 8), F32, gpu)          # a kept forward's rows go back in unchanged
        L_.check(L_.lib().ctrl_op_i2v_latent_encoder(L_.ptr(gk.view), None, L_.ptr(gs.view), L_.dtype_code(c.dt), L_.ptr(g2.view), None, c.B, c.F, c.HW, 1,
                                                     L_.cur_stream()))
        _untouched(c.id, gk, gs, g2)
        we.exact(c.id + " precomputed", g2.view, out)
    w.done()
    we.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# adaptive_avgpool_nhwc, unet_text_time
# ---------------------------------------------------------------------------------------------------------------------------
def test_adaptive_avgpool_nhwc(L_, gpu):
    """fp32 and fp16 on either side, OH != OW, output counts that are no multiple of 256; a one-element window (replication, the identity)
    is the conversion of its element, bit for bit"""
    w, we = Worst("adaptive_avgpool_nhwc"), Worst("adaptive_avgpool_nhwc one-element windows")
    for c in S.AAPOOL:
        x, ref, bound, one = S.aap_problem(c)
        gx, go = _inp(x, gpu), _out((ref.numel(),), c.y_dt, gpu)
        L_.check(L_.lib().ctrl_op_adaptive_avgpool_nhwc(L_.ptr(gx.view), L_.dtype_code(c.x_dt), L_.ptr(go.view), L_.dtype_code(c.y_dt), c.N, c.H, c.W, c.C,
                                                        c.OH, c.OW, L_.cur_stream()))
        _untouched(c.id, gx, go)
        out = go.view.cpu().reshape(ref.shape)
        w.close(c.id, out, ref, bound)
        if bool(one.any()):
            xi = x[:, [a for a, _ in S.aap_windows(c.H, c.OH)]][:, :, [a for a, _ in S.aap_windows(c.W, c.OW)]]
            we.exact(c.id, out[one], xi.float().to(c.y_dt)[one])
    w.done()
    we.done(True)


def test_unet_text_time(L_, gpu):
    """rows wider than the operand with poison between them; the text columns are the conversion to fp32, bit for bit; the sinusoids under
    helper_forms' sincos bound (its SC_C, SC_K)"""
    w, we = Worst("unet_text_time"), Worst("unet_text_time text")
    for c in S.TEXT_TIME:
        text, ids, ref, bound = S.tt_problem(c)
        width = c.text_dim + c.n_ids * c.dim
        gt, gi = _inp(text, gpu), _inp(ids, gpu)
        go = _out((c.B, width), F32, gpu, S.TT_PAD)
        L_.check(L_.lib().ctrl_op_unet_text_time(L_.ptr(gt.view), L_.dtype_code(c.dt), c.text_dim, L_.ptr(gi.view), c.n_ids, c.dim, L_.ptr(go.view),
                                                 width + S.TT_PAD, c.B, L_.cur_stream()))
        _untouched(c.id, gt, gi, go)
        out = go.view.cpu()
        we.exact(c.id, out[:, :c.text_dim].contiguous(), text.float())
        w.close(c.id, out[:, c.text_dim:], ref, bound)
    w.done()
    we.done(True)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(L_, gpu):
    """every refused call names the same poisoned buffer for all of its tensors: it comes back untouched"""
    g = Guarded.out((4096,), (slice(1024, 3072),), F32, gpu)
    ptr = g.view.data_ptr()
    assert ptr % 16 == 0
    for name, sym, args, msg in S.refusals(ptr, ptr + 4):
        rc = getattr(L_.lib(), sym)(*args, L_.cur_stream())
        err = (L_.lib().ctrl_last_error() or b"").decode()
        assert rc != 0 and msg in err, (name, rc, err)
    torch.cuda.synchronize()
    assert torch.equal(helpers._bits(g.buf), g._snap), "a refused call wrote"
