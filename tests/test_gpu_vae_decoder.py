"""KL-VAE decoder on the MI355X (csrc/vae.hip, csrc/plan_vae_decoder.cpp): the head and tail kernels against torch fp32, the tiny and the
SD / SDXL decoder against the fp32 restatement (tests/vae_decoder_ref.py, run on the GPU), batch invariance, graph replays, the refusal
of a first forward under capture, the encode -> decode round trip of the whole-VAE module, and the two pipeline helpers.

Measured on the MI355X (rel-inf against the fp32 restatement, bound 1e-3; fp32 module, seeded weights): tiny 2.0e-4; SD VAE latents
[1, 4, 64, 64] 1.7e-4, [2, 4, 64, 64] 2.0e-4, [1, 4, 72, 128] 1.1e-4, [1, 4, 128, 128] 9.6e-5; the tiny encode -> decode round trip
3.8e-4; head kernel 2e-7 .. 3e-7, tail kernel 5e-7 .. 1.1e-6.  tools/vae_decoder_bench.py times the plan against torch and prints torch-fp16's error on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_text_encoder import rel_inf
from vae_decoder_ref import SD_VAE, TINY, VaeDecoderRef, VaeRef, i2vgen_decode_latents, pil_to_u8, sdxl_decode_latents, seeded_latents
from vae_encoder_ref import seeded_pixels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOUND = 1e-3          # the project's parity bound (rel-inf against the fp32 restatement)
SEED = 2024


def _lib():
    from ctrl_adapter_amd import _lib
    return _lib


_MODELS = {}


def _pair(cfg_name):
    """(fp32 restatement on the GPU, mirror) with synthetic.seeded_init weights, built once per module"""
    if cfg_name not in _MODELS:
        import ctrl_adapter_amd as P
        from ctrl_adapter_amd.synthetic import seeded_init
        if cfg_name == "tiny_vae":
            ref = seeded_init(VaeRef(**TINY), seed=SEED).eval()
            m = P.AutoencoderKL(**TINY)
        else:
            cfg = {"tiny": TINY, "sd": SD_VAE}[cfg_name]
            ref = seeded_init(VaeDecoderRef(**cfg), seed=SEED).eval()
            m = P.AutoencoderKLDecoder(**cfg)
        m.load_state_dict(ref.state_dict())
        _MODELS[cfg_name] = (ref.to(DEV), m.to(DEV))
    return _MODELS[cfg_name]


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_head_kernel_matches_torch_fp32(dt, frames):
    """frames = 3: the latents are frame 1 of a [lat, 3, h, w] clip (channel stride 3 * h * w) whose other frames are NaN"""
    from ctrl_adapter_amd import ops
    lib = _lib()
    lat, h, w, C, s = 4, 13, 21, 64, 1.0 / 0.13025
    g = torch.Generator().manual_seed(7)
    clip = torch.full((lat, frames, h, w), float("nan"), dtype=dt, device=DEV)
    clip[:, frames // 2] = torch.randn(lat, h, w, generator=g).to(dt).to(DEV)
    zv = clip[:, frames // 2]                         # a view: [lat, h, w] with strides (frames * h * w, w, 1)
    z = zv.unsqueeze(0).contiguous()
    wpq = (torch.randn(lat, lat, 1, 1, generator=g) * 0.5).to(DEV)
    bpq = (torch.randn(lat, generator=g) * 0.1).to(DEV)
    win = (torch.randn(C, lat, 3, 3, generator=g) / 6.0).to(DEV)
    bin_ = (torch.randn(C, generator=g) * 0.1).to(DEV)
    want = F.conv2d(F.conv2d(z.float() * s, wpq, bpq), win, bin_, padding=1)
    out = torch.full((h * w + 3, C), float("nan"), device=DEV)
    wd = ops.pack_conv_w_direct(win)
    lib.check(lib.lib().ctrl_op_vae_dec_head(lib.ptr(zv), lib.dtype_code(dt), s, lib.ptr(wpq.reshape(lat, lat).contiguous()), lib.ptr(bpq),
                                             lib.ptr(wd), lib.ptr(bin_), lib.ptr(out), lat, h, w, zv.stride(0), C, lib.cur_stream()))
    got = out[:h * w].view(1, h, w, C).permute(0, 3, 1, 2)
    err = rel_inf(got, want)
    print("head %s frames %d rel-inf %.3e" % (dt, frames, err))
    assert err < 1e-5, err
    assert torch.isnan(out[h * w:]).all()           # nothing written past the map


def _tail(x_nhwc, gamma, beta, w, b, kind, odt, H, W, C):
    from ctrl_adapter_amd import ops
    lib = _lib()
    n = int(lib.lib().ctrl_op_gn_stats_floats(1, H * W, C, 32))
    st = torch.zeros(n, device=DEV)
    lib.check(lib.lib().ctrl_op_gn_stats(lib.ptr(x_nhwc), lib.F32, lib.ptr(st), 1, H * W, C, 32, lib.cur_stream()))
    wd = ops.pack_conv_w_direct(w)
    if kind == lib.VAE_DEC_SAMPLE:
        out = torch.full((3 * H * W + 64,), float("nan"), dtype=odt, device=DEV)
    elif kind == lib.VAE_DEC_UNIT:
        out = torch.full((3 * H * W + 64,), float("nan"), dtype=torch.float32, device=DEV)
    else:
        out = torch.full((3 * H * W + 64,), 77, dtype=torch.uint8, device=DEV)
    lib.check(lib.lib().ctrl_op_vae_dec_tail(lib.ptr(x_nhwc), lib.ptr(st), lib.ptr(gamma), lib.ptr(beta), 1e-6, lib.ptr(wd), lib.ptr(b), H, W,
                                             C, 3, kind, lib.ptr(out), lib.dtype_code(odt), lib.cur_stream()))
    tail_ = out[3 * H * W:]
    assert (tail_ == 77).all() if kind == lib.VAE_DEC_U8 else torch.isnan(tail_.float()).all()      # nothing written past the image
    body = out[:3 * H * W]
    return body.view(1, H, W, 3) if kind == lib.VAE_DEC_U8 else body.view(1, 3, H, W)


@pytest.mark.parametrize("C,H,W", [(32, 19, 45), (128, 40, 70), (128, 8, 32)])
def test_tail_kernel_matches_torch_fp32_and_postprocess_is_bit_exact(C, H, W):
    lib = _lib()
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(1, C, H, W, generator=g) * 1.5 + 0.3).to(DEV)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    w = (torch.randn(3, C, 3, 3, generator=g) / (9 * C) ** 0.5 * 1.5).to(DEV)
    b = (0.1 * torch.randn(3, generator=g)).to(DEV)
    want = F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, eps=1e-6)), w, b, padding=1)
    xh = x.permute(0, 2, 3, 1).contiguous()
    got = _tail(xh, gamma, beta, w, b, lib.VAE_DEC_SAMPLE, torch.float32, H, W, C)
    err = rel_inf(got, want)
    print("tail C%d %dx%d rel-inf %.3e" % (C, H, W, err))
    assert err < 1e-5, err
    assert (want / 2 + 0.5).min() < 0 and (want / 2 + 0.5).max() > 1          # both clamp edges are exercised
    for odt in (torch.float32, torch.float16, torch.bfloat16):
        s = _tail(xh, gamma, beta, w, b, lib.VAE_DEC_SAMPLE, odt, H, W, C)
        if odt != torch.float32:
            assert torch.equal(s, got.to(odt))                                    # .sample in the module's dtype: one rounding of the fp32 value
        unit = _tail(xh, gamma, beta, w, b, lib.VAE_DEC_UNIT, odt, H, W, C)
        want_unit = (s.float() / 2 + 0.5).clamp(0, 1)
        assert unit.dtype == torch.float32 and torch.equal(unit, want_unit)
        u8 = _tail(xh, gamma, beta, w, b, lib.VAE_DEC_U8, odt, H, W, C)
        want_u8 = (want_unit.cpu().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
        assert np.array_equal(u8.cpu().numpy(), want_u8)


def _check_decoder(ref, m, z):
    with torch.no_grad():
        want = ref.decode(z).sample
    got = m.decode(z).sample
    assert got.shape == want.shape and got.dtype == torch.float32
    err = rel_inf(got, want)
    print("decoder %s rel-inf %.3e  max|ref| %.3f" % (tuple(z.shape), err, want.abs().max().item()))
    assert err < BOUND, err
    return err


def test_tiny_decoder_matches_restatement():
    ref, m = _pair("tiny")
    _check_decoder(ref, m, seeded_latents(2, 24, 20, seed=1, device=DEV))


@pytest.mark.parametrize("N,h,w", [(1, 64, 64), (2, 64, 64), (1, 72, 128), (1, 128, 128)])
def test_sd_vae_decoder_matches_restatement(N, h, w):
    ref, m = _pair("sd")
    z = seeded_latents(N, h, w, seed=h + N, device=DEV)
    _check_decoder(ref, m, z)
    torch.cuda.empty_cache()


def test_batch_invariance():
    ref, m = _pair("sd")
    z = seeded_latents(2, 32, 32, seed=9, device=DEV)
    both = m.run(z)
    for i in range(2):
        assert torch.equal(both[i:i + 1], m.run(z[i:i + 1].clone()))
    lib = _lib()
    u8 = m.run(z, lib.VAE_DEC_U8)
    for i in range(2):
        assert torch.equal(u8[i:i + 1], m.run(z[i:i + 1].clone(), lib.VAE_DEC_U8))


def test_graph_replay_is_bit_identical():
    _, m = _pair("tiny")
    z = seeded_latents(2, 16, 16, seed=3, device=DEV)
    eager = m.run(z)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.run(z)                       # warm: the workspace of this size exists
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.run(z)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_first_forward_of_a_new_size_under_capture_is_refused():
    import ctrl_adapter_amd as P
    ref, _ = _pair("tiny")
    m = P.AutoencoderKLDecoder(**TINY)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV)
    small, large = seeded_latents(1, 8, 8, seed=1, device=DEV), seeded_latents(1, 40, 40, seed=2, device=DEV)
    m.run(small)                       # the plan and a small workspace exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot run under stream capture"):
        with torch.cuda.graph(g):
            m.run(large)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = ref.decode(large).sample
    assert rel_inf(m.run(large), want) < BOUND      # eagerly it allocates and runs


def test_latent_dtypes_and_scale():
    ref, m = _pair("tiny")
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        z = seeded_latents(1, 12, 20, seed=4, device=DEV).to(dt)
        with torch.no_grad():
            want = ref.decode(z.float() * 2.5).sample
        assert rel_inf(m.run(z, scale=2.5, out_dtype=torch.float32), want) < BOUND


def test_whole_vae_round_trip_matches_restatement():
    ref, m = _pair("tiny_vae")
    x = seeded_pixels(1, 256, 256, seed=5, device=DEV)
    with torch.no_grad():
        zr = ref.encode(x).latent_dist.mode()
        want = ref.decode(zr).sample
    zm = m.encode(x).latent_dist.mode()
    assert rel_inf(zm, zr) < BOUND
    got = m.decode(zm).sample
    err = rel_inf(got, want)
    print("round trip rel-inf %.3e" % err)
    assert got.shape == (1, 3, 256, 256) and err < BOUND, err
    assert m.config.force_upcast is False


def test_pipeline_helpers_match_restated_methods():
    import ctrl_adapter_amd as P
    ref, m = _pair("tiny")
    sf = ref.config.scaling_factor
    # latents scaled so that the image stays inside the range where one 8-bit level is wider than the parity bound allows an error
    z = seeded_latents(2, 24, 16, seed=6, device=DEV) * 0.5
    lat = z * sf
    with torch.no_grad():
        pre = ref.decode(lat / sf).sample
        want_pt = sdxl_decode_latents(ref, lat, "pt")
        want_u8 = sdxl_decode_latents(ref, lat, "pil")
    peak = pre.abs().max().item()
    print("helper pre-clamp max|ref| %.3f" % peak)
    assert BOUND * peak * 127.5 < 1.0          # an error of 1e-3 * max|ref| moves x / 2 + 0.5 by less than one level of 255
    got_pt = P.decode_sdxl_latents(m, lat, "pt")
    assert got_pt.shape == want_pt.shape and got_pt.dtype == torch.float32
    tol_pt = BOUND * max(1.0, peak / 2)         # x / 2 + 0.5 halves the error of x, which the parity bound holds below 1e-3 * max|ref|
    assert (got_pt - want_pt).abs().max().item() < tol_pt
    got_np = P.decode_sdxl_latents(m, lat, "np")
    assert got_np.shape == (2, 48, 32, 3) and np.array_equal(got_np, got_pt.cpu().permute(0, 2, 3, 1).numpy())
    pil = P.decode_sdxl_latents(m, lat, "pil")
    assert len(pil) == 2 and pil[0].size == (32, 48)
    diff = np.abs(pil_to_u8(pil).astype(np.int32) - want_u8.astype(np.int32))
    print("pil levels off: max %d, pixels off %d of %d" % (diff.max(), int((diff > 0).sum()), diff.size))
    assert diff.max() <= 1
    # I2VGen-XL: [B, C, F, h, w] -> [B, 3, F, H, W] float32, chunk size that does not divide B * F
    lat5 = torch.randn(2, 4, 3, 10, 12, generator=torch.Generator().manual_seed(8)).to(DEV) * sf
    with torch.no_grad():
        want = i2vgen_decode_latents(ref, lat5, decode_chunk_size=4)
    got = P.decode_i2vgen_latents(m, lat5, decode_chunk_size=4)
    assert got.shape == want.shape == (2, 3, 3, 20, 24) and got.dtype == torch.float32
    assert rel_inf(got, want) < BOUND
    # the whole-VAE module takes the same route
    _, vae = _pair("tiny_vae")
    refv, _ = _pair("tiny_vae")
    with torch.no_grad():
        want = sdxl_decode_latents(refv, lat, "pt")
    assert (P.decode_sdxl_latents(vae, lat, "pt") - want).abs().max().item() < tol_pt


def test_strided_latents_equal_their_dense_copy():
    """the frames of a [C, F, h, w] clip as the [F, C, h, w] view the I2VGen-XL helper passes (image stride h * w, channel stride
    F * h * w) decode to the bits of their contiguous copy"""
    ref, m = _pair("tiny")
    lat = TINY["latent_channels"]
    clip = torch.randn(lat, 3, 6, 10, generator=torch.Generator().manual_seed(5)).to(DEV)
    view = clip.transpose(0, 1)
    assert not view.is_contiguous()
    assert torch.equal(m.run(view), m.run(view.contiguous()))
