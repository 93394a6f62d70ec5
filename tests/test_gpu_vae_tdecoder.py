"""Temporal KL-VAE decoder on the MI355X (csrc/plan_vae_tdecoder.cpp, csrc/vae.hip): the time-conv kernel against F.conv3d in fp32 with
its three epilogues, the tiny and the SD-VAE-config temporal decoder against the fp32 restatement (tests/vae_tdecoder_ref.py, run on the
GPU) at every frame-group size, clip invariance, decode_svd_latents, graph replays, the refusal of a first forward under capture, and
the encode -> decode round trip of the whole-VAE module.

Measured on the MI355X (rel-inf against the fp32 restatement, bound 1e-3; fp32 module, seeded weights, mix factors -1.5 / 0.5 / 2.0):
tiny (layers_per_block 1: no mid attention runs) latents [F, 4, 12, 10]: F = 1 8.6e-7, F = 2 9.3e-7, F = 5 1.0e-6, the same for
frames_per_launch None / 1 / 2; tiny with layers_per_block 2 (the mid attention, fp16 Q / K / V / P) [3, 4, 12, 10] 1.4e-4; the SD VAE
config [3, 4, 16, 24] 1.0e-4 at frames_per_launch None and 1; decode_svd_latents (tiny, B = 2, F = 3, chunks of 4) 9.1e-7; the tiny
encode -> decode round trip 2.7e-4; the time-conv kernel alone 6e-8 .. 2.1e-7 against F.conv3d (bound 1e-5).
tools/vae_tdecoder_bench.py times the plan against torch and prints torch-fp16's error on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_text_encoder import rel_inf
from vae_decoder_ref import seeded_latents
from vae_encoder_ref import seeded_pixels
from vae_tdecoder_ref import SD_VAE, TINY, VaeTemporalRef, seeded_tdecoder, svd_decode_latents

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOUND = 1e-3          # the project's parity bound (rel-inf against the fp32 restatement)
SEED = 2025
TINY2 = dict(block_out_channels=(32, 64), layers_per_block=2, latent_channels=4)      # the mid block with its attention


def _lib():
    from ctrl_adapter_amd import _lib
    return _lib


_MODELS = {}


def _pair(cfg_name):
    """(fp32 restatement on the GPU, mirror) with synthetic.seeded_init weights and distinct mix factors, built once per module"""
    if cfg_name not in _MODELS:
        import ctrl_adapter_amd as P
        cfg = {"tiny": TINY, "tiny2": TINY2, "sd": SD_VAE}[cfg_name]
        ref = seeded_tdecoder(VaeTemporalRef, cfg, SEED)
        m = P.AutoencoderKLTemporalDecoder(**cfg)
        m.load_state_dict(ref.state_dict())
        _MODELS[cfg_name] = (ref.to(DEV), m.to(DEV))
    return _MODELS[cfg_name]


# ------------------------------------------------------------------------------------------------------------------ the time-conv kernel
def _time_conv(x, w, b, kind, odt, misalign=0):
    """ctrl_op_vae_time_conv on x [F, oc, H, W] fp32 inside a poisoned buffer (NaN / 77 behind the output)"""
    lib = _lib()
    Fr, oc, H, W = x.shape
    n = Fr * oc * H * W
    if kind == lib.VAE_DEC_U8:
        buf = torch.full((misalign + n + 64,), 77, dtype=torch.uint8, device=DEV)
    else:
        buf = torch.full((misalign + n + 64,), float("nan"), dtype=torch.float32 if kind == lib.VAE_DEC_UNIT else odt, device=DEV)
    out = buf[misalign:]
    lib.check(lib.lib().ctrl_op_vae_time_conv(lib.ptr(x), lib.ptr(w), lib.ptr(b), Fr, H, W, oc, kind, lib.ptr(out), lib.dtype_code(odt),
                                              lib.cur_stream()))
    tail_, head_ = out[n:], buf[:misalign]
    if kind == lib.VAE_DEC_U8:
        assert (tail_ == 77).all() and (head_ == 77).all()            # nothing written outside the frames
        return out[:n].view(Fr, H, W, oc)
    assert torch.isnan(tail_.float()).all() and torch.isnan(head_.float()).all()
    return out[:n].view(Fr, oc, H, W)


@pytest.mark.parametrize("H,W", [(13, 21), (16, 24)], ids=["13x21_scalar", "16x24_vector"])
@pytest.mark.parametrize("Fr", [1, 2, 5])
def test_time_conv_kernel_matches_conv3d_fp32_and_postprocess_is_bit_exact(Fr, H, W):
    lib = _lib()
    oc = 3
    g = torch.Generator().manual_seed(100 * Fr + H)
    x = (torch.randn(Fr, oc, H, W, generator=g) * 1.5).to(DEV)
    w = (torch.randn(oc, oc, 3, 1, 1, generator=g) * 0.5).to(DEV)
    b = (torch.randn(oc, generator=g) * 0.1).to(DEV)
    want = F.conv3d(x.cpu().permute(1, 0, 2, 3)[None], w.cpu(), b.cpu(), padding=(1, 0, 0))[0].permute(1, 0, 2, 3)
    got = _time_conv(x, w, b, lib.VAE_DEC_SAMPLE, torch.float32)
    err = rel_inf(got, want)
    print("time conv F%d %dx%d rel-inf %.3e" % (Fr, H, W, err))
    assert err < 1e-5, err
    assert (want / 2 + 0.5).min() < 0 and (want / 2 + 0.5).max() > 1          # both clamp edges are exercised
    for odt in (torch.float32, torch.float16, torch.bfloat16):
        s = _time_conv(x, w, b, lib.VAE_DEC_SAMPLE, odt)
        if odt != torch.float32:
            assert torch.equal(s, got.to(odt))                                    # one rounding of the fp32 value
        unit = _time_conv(x, w, b, lib.VAE_DEC_UNIT, odt)
        want_unit = (s.float() / 2 + 0.5).clamp(0, 1)
        assert unit.dtype == torch.float32 and torch.equal(unit, want_unit)
        u8 = _time_conv(x, w, b, lib.VAE_DEC_U8, odt)
        want_u8 = (want_unit.cpu().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
        assert np.array_equal(u8.cpu().numpy(), want_u8)
    # an output that is not 16-byte aligned takes the scalar path: the same bits
    assert torch.equal(_time_conv(x, w, b, lib.VAE_DEC_SAMPLE, torch.float32, misalign=1), got)
    assert torch.equal(_time_conv(x, w, b, lib.VAE_DEC_U8, torch.float32, misalign=1), _time_conv(x, w, b, lib.VAE_DEC_U8, torch.float32))


# ------------------------------------------------------------------------------------------------------------------ the decoder
_WANT = {}


def _want(cfg_name, Fr, h, w):
    """the restatement's decode of the seeded latents as one clip of Fr frames, computed once"""
    key = (cfg_name, Fr, h, w)
    if key not in _WANT:
        ref, _ = _pair(cfg_name)
        z = seeded_latents(Fr, h, w, seed=10 * Fr + h, device=DEV)
        with torch.no_grad():
            _WANT[key] = (z, ref.decode(z, Fr).sample)
    return _WANT[key]


def _check(cfg_name, Fr, h, w, fpl):
    _, m = _pair(cfg_name)
    z, want = _want(cfg_name, Fr, h, w)
    got = m.run_decoder(z, Fr, frames_per_launch=fpl)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = rel_inf(got, want)
    print("tdecoder %s F%d %dx%d frames_per_launch %s rel-inf %.3e  max|ref| %.3f" % (cfg_name, Fr, h, w, fpl, err, want.abs().max().item()))
    assert err < BOUND, err


@pytest.mark.parametrize("fpl", [None, 1, 2])
@pytest.mark.parametrize("Fr", [1, 2, 5])
def test_tiny_temporal_decoder_matches_restatement(Fr, fpl):
    """latents 12 x 10: 120 and 480 rows per frame, so the 64- to 256-row GEMM tiles straddle frame boundaries"""
    _check("tiny", Fr, 12, 10, fpl)


@pytest.mark.parametrize("fpl", [None, 2])
def test_tiny_temporal_decoder_with_the_mid_attention_matches_restatement(fpl):
    _check("tiny2", 3, 12, 10, fpl)


@pytest.mark.parametrize("fpl", [None, 1])
def test_sd_vae_temporal_decoder_matches_restatement(fpl):
    """the SVD VAE's widths: the 256- and 512-channel temporal convs"""
    _check("sd", 3, 16, 24, fpl)
    torch.cuda.empty_cache()


def test_two_clips_in_one_call_equal_the_clips_alone():
    _, m = _pair("tiny")
    z = seeded_latents(4, 12, 10, seed=9, device=DEV)
    both = m.run_decoder(z, 2)
    for i in range(2):
        assert torch.equal(both[2 * i:2 * i + 2], m.run_decoder(z[2 * i:2 * i + 2].clone(), 2))
    lib = _lib()
    u8 = m.run_decoder(z, 2, lib.VAE_DEC_U8)
    assert u8.shape == (4, 24, 20, 3) and u8.dtype == torch.uint8
    want = (both / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(u8.cpu().numpy(), (want * 255).round().astype("uint8"))


def test_decode_svd_latents_matches_restated_method():
    import ctrl_adapter_amd as P
    ref, m = _pair("tiny")
    sf = ref.config.scaling_factor
    lat = torch.randn(2, 3, 4, 10, 12, generator=torch.Generator().manual_seed(8)).to(DEV) * sf
    with torch.no_grad():
        want = svd_decode_latents(ref, lat, 3, decode_chunk_size=4)
    got = P.decode_svd_latents(m, lat, 3, decode_chunk_size=4)
    assert got.shape == want.shape == (2, 3, 3, 20, 24) and got.dtype == torch.float32
    err = rel_inf(got, want)
    print("decode_svd_latents rel-inf %.3e" % err)
    assert err < BOUND, err


def test_first_forward_of_a_new_size_under_capture_is_refused_then_replays_are_bit_identical():
    import ctrl_adapter_amd as P
    ref, _ = _pair("tiny")
    m = P.AutoencoderKLTemporalDecoder(**TINY)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV)
    small, z = seeded_latents(1, 6, 6, seed=1, device=DEV), seeded_latents(3, 12, 10, seed=2, device=DEV)
    m.run_decoder(small, 1)            # the plan and a small workspace exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot run under stream capture"):
        with torch.cuda.graph(g):
            m.run_decoder(z, 3)
    torch.cuda.synchronize()
    eager = m.run_decoder(z, 3)        # eagerly it allocates and runs
    with torch.no_grad():
        assert rel_inf(eager, ref.decode(z, 3).sample) < BOUND
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):          # one stream, no branches
        out = m.run_decoder(z, 3)
    for _ in range(3):
        out.zero_()                    # what the replay writes, not what the capture left
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_whole_vae_round_trip_matches_restatement():
    ref, m = _pair("tiny")
    x = seeded_pixels(2, 64, 48, seed=5, device=DEV)
    with torch.no_grad():
        zr = ref.encode(x).latent_dist.mode()
        want = ref.decode(zr, 2).sample
        want_fwd = ref(x, num_frames=2).sample
    zm = m.encode(x).latent_dist.mode()
    assert rel_inf(zm, zr) < BOUND
    got = m.decode(zm, num_frames=2).sample
    err = rel_inf(got, want)
    print("round trip rel-inf %.3e" % err)
    assert got.shape == (2, 3, 64, 48) and err < BOUND, err
    assert rel_inf(m(x, num_frames=2).sample, want_fwd) < BOUND
    assert m.config.force_upcast is False
