"""CLIP vision tower on the MI355X (csrc/vision.hip, csrc/plan_vision.cpp): the patch, embed and resize kernels against torch and the
golden, the tower against transformers (tests/golden/clip_vision.pt) and, at full ViT-H/14 depth, against the fp32 restatement
(tests/clip_vision_ref.py), batch invariance in both GEMM forms, graph replays, output dtypes, encode_svd_image from a PIL image, and the
embedding driving the video ControlNetAdapter."""
import os
import sys

import numpy as np
import pytest
import torch

from clip_vision_ref import TINY, VIT_H, CLIPVisionRef, seeded_pixels, svd_preprocess
from helpers import check_digest
from test_gpu_text_encoder import rel_inf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# ViT-H/14 at 32 layers against the fp32 restatement: the project's bound
BOUND = 1e-3
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vision.pt")


def _lib():
    from ctrl_adapter_amd import _lib
    return _lib


def _ms():
    import ctypes
    return (ctypes.c_float * 6)(*(MEAN + STD))


def _seeded_ref(cfg):
    from ctrl_adapter_amd.synthetic import seeded_init
    from make_clip_vision_golden import WEIGHT_SEED
    return seeded_init(CLIPVisionRef(**cfg), seed=WEIGHT_SEED).eval()


def _mirror(ref, cfg, gemm_form=None, dtype=torch.float32):
    import ctrl_adapter_amd as P
    m = P.CLIPVisionModelWithProjection(**cfg, gemm_form=gemm_form)
    m.load_state_dict(ref.state_dict())
    return m.to(dtype).to(DEV)


def _im2col(x, p):
    N, C_, S, _ = x.shape
    G = S // p
    cols = x.reshape(N, C_, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(N * G * G, C_ * p * p)
    K = C_ * p * p
    return torch.nn.functional.pad(cols, (0, (K + 63) // 64 * 64 - K))


@pytest.mark.parametrize("kind", ["f32_norm", "u8_norm", "f16_plain", "bf16_norm"])
def test_patchify_is_torch_normalise_then_cast(kind):
    L_ = _lib()
    S, p, N = 224, 14, 3
    g = torch.Generator().manual_seed(3)
    m = torch.tensor(MEAN).view(1, 3, 1, 1)
    s = torch.tensor(STD).view(1, 3, 1, 1)
    if kind == "u8_norm":
        u8 = torch.randint(0, 256, (N, S, S, 3), generator=g, dtype=torch.uint8)
        src, dt = u8, L_.U8_NHWC
        want = ((u8.permute(0, 3, 1, 2).float() / 255.0 - m) / s).half()
    else:
        x = torch.rand(N, 3, S, S, generator=g)
        tdt = {"f32_norm": torch.float32, "f16_plain": torch.float16, "bf16_norm": torch.bfloat16}[kind]
        src, dt = x.to(tdt), L_.dtype_code(tdt)
        want = src.half() if kind == "f16_plain" else ((src.float() - m) / s).half()
    Kpad = 640
    out = torch.full(((S // p) ** 2 * N, Kpad), float("nan"), dtype=torch.float16, device=DEV)
    d = src.contiguous().to(DEV)
    L_.check(L_.lib().ctrl_op_vision_patchify(L_.ptr(d), dt, N, S, p, None if kind == "f16_plain" else _ms(), L_.ptr(out), Kpad,
                                              L_.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _im2col(want, p))


def test_embed_and_two_layernorms_match_fp32_torch():
    L_ = _lib()
    N, Lt, C_ = 2, 257, 1280
    g = torch.Generator().manual_seed(4)
    patch, cls, pos = torch.randn(N * (Lt - 1), C_, generator=g), torch.randn(C_, generator=g), torch.randn(Lt, C_, generator=g)
    g0, b0, g1, b1 = (1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g),
                      1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g))
    dv = [t.to(DEV) for t in (patch, cls, pos, g0, b0, g1, b1)]
    x = torch.empty(N * Lt, C_, device=DEV)
    y = torch.empty(N * Lt, C_, dtype=torch.float16, device=DEV)
    L_.check(L_.lib().ctrl_op_vision_embed(*[L_.ptr(t) for t in dv[:3]], N, Lt, C_, *[L_.ptr(t) for t in dv[3:]], 1e-5, L_.ptr(x), L_.ptr(y),
                                           L_.cur_stream()))
    torch.cuda.synchronize()
    e = torch.cat([cls.view(1, 1, -1).expand(N, 1, C_), patch.view(N, Lt - 1, C_)], 1) + pos[None]
    wx = torch.nn.functional.layer_norm(e, (C_,), g0, b0, 1e-5)
    wy = torch.nn.functional.layer_norm(wx, (C_,), g1, b1, 1e-5)
    ex, ey = rel_inf(x.view(N, Lt, C_), wx), rel_inf(y.view(N, Lt, C_), wy)
    print("vision_embed: x rel-inf %.2e, y rel-inf %.2e" % (ex, ey))
    assert ex <= 2e-6 and ey <= 1e-3


@pytest.mark.parametrize("case", range(4))
def test_resize_kernel_matches_the_pipeline_helper(case):
    from ctrl_adapter_amd.vision_encoder import clip_resize_aa
    c = torch.load(GOLDEN, weights_only=False)["resize"][case]
    g = torch.Generator().manual_seed(c["seed"])
    u8 = torch.randint(0, 256, (1, c["H"], c["W"], 3), generator=g, dtype=torch.uint8)
    outs = [clip_resize_aa(u8.to(DEV)), clip_resize_aa(u8.float().div(255.0).permute(0, 3, 1, 2).contiguous().to(DEV))]
    torch.cuda.synchronize()
    d = c["out"]
    for out in outs:
        y = (out.cpu() * 2.0 - 1.0).reshape(-1)[::d["step"]][:4096]
        err = (y - d["samples"]).abs().max().item()
        print("clip_resize_aa %dx%d: max abs %.2e" % (c["H"], c["W"], err))
        assert err <= 2e-6
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("act", ["quick", "gelu"])
@pytest.mark.parametrize("form", [0, 1])
def test_tiny_tower_matches_transformers(act, form):
    g = torch.load(GOLDEN, weights_only=False)
    cfg = dict(TINY, hidden_act="quick_gelu" if act == "quick" else "gelu")
    rec = g["tiny_" + act]
    m = _mirror(_seeded_ref(cfg), cfg, form)
    px = seeded_pixels(rec["N"], cfg["image_size"], seed=rec["pixels_seed"]).to(DEV)
    r = m(px, output_hidden_states=True)
    _, pooled, _, _ = m.run(px, pooled=True, embeds=False)
    torch.cuda.synchronize()
    errs = {k: rel_inf(t, rec[k]["full"]) for k, t in (("image_embeds", r.image_embeds), ("last", r.last_hidden_state),
                                                        ("penultimate", r.hidden_states[-2]), ("pooled", pooled))}
    print("tiny %s form %d: %s" % (act, form, " ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= 2e-3


@pytest.fixture(scope="module")
def vith2():
    g = torch.load(GOLDEN, weights_only=False)
    return g, _seeded_ref(g["vith_cfg"])


@pytest.mark.parametrize("form", [0, 1])
def test_vit_h_two_layers_match_golden_digests(vith2, form):
    g, ref = vith2
    rec = g["vith"]
    m = _mirror(ref, g["vith_cfg"], form)
    px = seeded_pixels(rec["N"], 224, seed=rec["pixels_seed"]).to(DEV)
    r = m(px, output_hidden_states=True)
    torch.cuda.synchronize()
    e = [check_digest(r.image_embeds, rec["image_embeds"], 2e-3, "image_embeds"), check_digest(r.last_hidden_state, rec["last"], 2e-3, "last"),
         check_digest(r.hidden_states[-2], rec["penultimate"], 2e-3, "penultimate")]
    print("ViT-H 2 layers form %d vs transformers: embeds %.2e last %.2e penultimate %.2e" % ((form,) + tuple(e)))


@pytest.mark.parametrize("form", [0, 1])
def test_batch_invariance(vith2, form):
    g, ref = vith2
    m = _mirror(ref, g["vith_cfg"], form, torch.float16)
    px = seeded_pixels(4, 224, seed=9).half().to(DEV)
    four = m.run(px, last=True, pooled=True, embeds=True)
    for i in range(4):
        one = m.run(px[i:i + 1].contiguous(), last=True, pooled=True, embeds=True)
        for a, b in zip(one[:3], four[:3]):
            assert torch.equal(a[0], b[i]), "image %d differs alone vs inside a batch of 4 (form %d)" % (i, form)


def test_graph_replays_are_bit_identical(vith2):
    g, ref = vith2
    m = _mirror(ref, g["vith_cfg"], 0, torch.float16)
    px = seeded_pixels(2, 224, seed=10).half().to(DEV)
    eager = m(px).image_embeds.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(px)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(px).image_embeds
    for _ in range(20):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_output_dtypes(vith2, dt):
    g, ref = vith2
    m = _mirror(ref, g["vith_cfg"], 0, dt)
    px = seeded_pixels(1, 224, seed=11).to(dt).to(DEV)
    r = m(px, output_hidden_states=True)
    assert r.image_embeds.dtype == dt and r.last_hidden_state.dtype == dt and r.hidden_states[0].dtype == dt
    assert next(m.parameters()).dtype == dt
    want = ref.to(DEV)(px.float()).image_embeds
    ref.cpu()
    e = rel_inf(r.image_embeds, want)
    print("output dtype %s: image_embeds rel-inf %.2e" % (dt, e))
    assert e <= (2e-3 if dt == torch.float32 else 1e-2)


@pytest.fixture(scope="module")
def vith_full():
    ref = _seeded_ref(VIT_H)
    m = _mirror(ref, VIT_H, None)
    return ref.to(DEV), m


@pytest.mark.parametrize("B", [1, 2])
def test_full_vit_h_against_fp32_restatement(vith_full, B):
    ref, m = vith_full
    px = seeded_pixels(B, 224, seed=20 + B).to(DEV)
    r = m(px)
    with torch.no_grad():
        w = ref(px)
    torch.cuda.synchronize()
    ee, el = rel_inf(r.image_embeds, w.image_embeds), rel_inf(r.last_hidden_state, w.last_hidden_state)
    print("ViT-H/14 32 layers B=%d vs fp32 restatement: image_embeds rel-inf %.3e, last_hidden_state rel-inf %.3e (bound %.0e)"
          % (B, ee, el, BOUND))
    assert ee <= BOUND and el <= BOUND


@pytest.fixture(scope="module")
def svd_small():
    cfg = dict(TINY, image_size=224, projection_dim=1024)
    ref = _seeded_ref(cfg)
    return cfg, ref, _mirror(ref, cfg, None, torch.float16)


def test_encode_svd_image_from_pil_matches_restated_pipeline(svd_small):
    PIL = pytest.importorskip("PIL.Image")
    import ctrl_adapter_amd as P
    cfg, ref, m = svd_small
    arr = np.random.default_rng(5).integers(0, 256, (576, 1024, 3), dtype=np.uint8)

    class FE:
        image_mean, image_std = list(MEAN), list(STD)
    out = P.encode_svd_image(m, FE(), PIL.fromarray(arr), DEV, 2, True)
    pix = svd_preprocess(arr[None], MEAN, STD)
    with torch.no_grad():
        want = ref(pix.half().float()).image_embeds
    torch.cuda.synchronize()
    assert out.shape == (4, 1, 1024) and out.dtype == torch.float16
    assert torch.count_nonzero(out[:2]) == 0 and torch.equal(out[2], out[3])
    e = rel_inf(out[2, 0], want[0])
    print("encode_svd_image (576x1024 PIL) vs the restated pipeline: rel-inf %.2e" % e)
    assert e <= 2e-3


def test_embedding_drives_the_video_adapter(svd_small):
    PIL = pytest.importorskip("PIL.Image")
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import cases
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    cfg, ref, m = svd_small
    arr = np.random.default_rng(6).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    emb = P.encode_svd_image(m, None, PIL.fromarray(arr), DEV, 1, False)
    with torch.no_grad():
        emb_ref = ref(svd_preprocess(arr[None], MEAN, STD)).image_embeds.unsqueeze(1)
    ad = seeded_init(P.ControlNetAdapter(**cases.ADAPTER_VIDEO), seed=33).to(DEV)
    downs, midin = cases.pyramid_inputs(N=8, h0=8, seed=300, with_mid=True)
    kw = dict(mid_block_res_sample=midin.half().to(DEV), num_frames=4, timestep=torch.tensor(961.0))
    out, _ = ad([d.half().to(DEV) for d in downs], encoder_hidden_states=emb.half(), **kw)
    out_ref, _ = ad([d.half().to(DEV) for d in downs], encoder_hidden_states=emb_ref.half().to(DEV), **kw)
    torch.cuda.synchronize()
    worst = max(rel_inf(a, b) for a, b in zip(out, out_ref) if a is not None and b.abs().max() > 0)
    e_in = rel_inf(emb, emb_ref)
    bound = max(BOUND, 2.5 * e_in)
    print("video adapter on the HIP image embedding vs the restatement's: worst rel-inf %.2e (embedding %.2e, bound %.2e)"
          % (worst, e_in, bound))
    assert worst <= bound
