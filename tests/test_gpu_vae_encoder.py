"""KL-VAE encoder on the MI355X (csrc/vae.hip, csrc/plan_vae.cpp): the tap-origin convolution of the implicit GEMM against F.pad + F.conv2d,
the row softmax and the posterior kernel against torch, the tiny and the SD / SVD encoder against the fp32 restatement
(tests/vae_encoder_ref.py, run on the GPU), batch invariance, graph replays, pixel dtypes, and the two pipeline helpers."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_text_encoder import rel_inf
from vae_encoder_ref import SD_VAE, TINY, VaeEncoderRef, i2vgen_prepare_image_latents, seeded_pixels, svd_encode_vae_image

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
        cfg = {"tiny": TINY, "sd": SD_VAE}[cfg_name]
        ref = seeded_init(VaeEncoderRef(**cfg), seed=SEED).eval()
        m = P.AutoencoderKLEncoder(**cfg)
        m.load_state_dict(ref.state_dict())
        _MODELS[cfg_name] = (ref.to(DEV), m.to(DEV))
    return _MODELS[cfg_name]


@pytest.mark.parametrize("cin,N,H,W", [(128, 2, 32, 32), (256, 2, 24, 40), (512, 2, 16, 16)])
def test_tap_origin_conv_is_pad_then_stride2_conv(cin, N, H, W):
    from ctrl_adapter_amd import ops
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(N, cin, H, W, generator=g).half().float()
    w = (torch.randn(cin, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half().float()
    b = torch.randn(cin, generator=g) * 0.1
    xh = x.permute(0, 2, 3, 1).contiguous().half().to(DEV)
    wp = ops.pack_conv_w(w.to(DEV))
    bd = b.to(DEV)

    def run(origin):
        pads = 1 if origin else 2
        Ho, Wo = (H + pads - 3) // 2 + 1, (W + pads - 3) // 2 + 1
        out = torch.empty(N, Ho, Wo, cin, dtype=torch.float32, device=DEV)
        geom = dict(Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=2, up=1)
        ops.igemm(xh, cin, wp, N * Ho * Wo, cin, cin, taps=9, mode=ops.IG_CONV2D, geom=geom, bias=bd, rows_per_img=Ho * Wo,
                  segs=[(out, cin, 0, cin, ops.SEG_ROW, 1)], tap_origin=origin)
        return out.permute(0, 3, 1, 2).cpu()

    want1 = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    got1 = run(1)
    assert got1.shape == want1.shape == (N, cin, H // 2, W // 2)
    assert rel_inf(got1, want1) < 1e-5
    want0 = F.conv2d(x, w, b, stride=2, padding=1)
    got0 = run(0)
    assert rel_inf(got0, want0) < 1e-5
    # origin 0 is today's descriptor: a zero-initialised field (ops.igemm's default) takes exactly the same path
    Ho, Wo = got0.shape[2], got0.shape[3]
    out = torch.empty(N, Ho, Wo, cin, dtype=torch.float32, device=DEV)
    ops.igemm(xh, cin, wp, N * Ho * Wo, cin, cin, taps=9, mode=ops.IG_CONV2D, geom=dict(Hin=H, Win=W, Hout=Ho, Wout=Wo, stride=2, up=1),
              bias=bd, rows_per_img=Ho * Wo, segs=[(out, cin, 0, cin, ops.SEG_ROW, 1)])
    assert torch.equal(out.permute(0, 3, 1, 2).cpu(), got0)


@pytest.mark.parametrize("L", [4096, 9216, 16384])
def test_row_softmax_matches_torch_fp32(L):
    lib = _lib()
    rows, Lpad = 48, (L + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(L)
    S = torch.randn(rows, L + 16, device=DEV, generator=g) * 6.0
    P = torch.full((rows, Lpad), float("nan"), dtype=torch.float16, device=DEV)
    lib.check(lib.lib().ctrl_op_vae_row_softmax(lib.ptr(S), L + 16, lib.ptr(P), Lpad, rows, L, Lpad, lib.cur_stream()))
    want = torch.softmax(S[:, :L], dim=1)
    got = P[:, :L].float()
    assert ((got - want).abs() <= want * 1e-3 + 1e-7).all()
    assert (P[:, L:] == 0).all()


@pytest.mark.parametrize("odt", [torch.float32, torch.float16, torch.bfloat16])
def test_posterior_kernel_at_clamp_edges(odt):
    lib = _lib()
    lat, N, h, w = 4, 2, 3, 5
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N * h * w, 16, generator=g)
    wq = torch.eye(8) + 0.01 * torch.randn(8, 8, generator=g)
    bq = torch.zeros(8)
    edges = torch.tensor([-45.0, -30.0, -0.5, 20.0, 31.0])
    x[:, 4:8] = edges.repeat(N * h * w * 4 // 5 + 1)[:N * h * w * 4].view(-1, 4)
    eps = torch.randn(N, lat, h, w, generator=g)
    q = (x[:, :8] @ wq.T + bq).view(N, h, w, 8).permute(0, 3, 1, 2)
    mean, logvar = q[:, :4], q[:, 4:].clamp(-30, 20)
    assert (logvar == -30).any() and (logvar == 20).any()
    want = {0: mean * 0.5, 1: (mean + torch.exp(0.5 * logvar) * eps) * 0.5,
            2: torch.cat([mean, logvar, torch.exp(0.5 * logvar), torch.exp(logvar)], 1)}
    xd, wqd, bqd, ed = x.to(DEV), wq.to(DEV), bq.to(DEV), eps.to(DEV)
    for kind, ref in want.items():
        out = torch.empty(ref.shape, dtype=odt, device=DEV)
        lib.check(lib.lib().ctrl_op_vae_posterior(lib.ptr(xd), 16, 0, lib.ptr(wqd), lib.ptr(bqd), N, lat, h, w, lib.ptr(ed), lib.F32, 0.5,
                                                  kind, lib.ptr(out), lib.dtype_code(odt), lib.cur_stream()))
        tol = 1e-5 if odt == torch.float32 else (1e-3 if odt == torch.float16 else 8e-3)
        got, refc = out.float().cpu(), ref.to(odt).float()       # torch's own rounding of the fp32 result (inf beyond fp16's range)
        close = (got - refc).abs() <= refc.abs() * tol + tol * mean.abs().max()
        assert ((got == refc) | close).all(), (kind, odt)


def _check_encoder(ref, m, x, eps_seed=5):
    with torch.no_grad():
        dist_r = ref.encode(x).latent_dist
    dist_m = m.encode(x).latent_dist
    err = rel_inf(dist_m.mode(), dist_r.mode())
    assert err < BOUND, err
    assert rel_inf(dist_m.std, dist_r.std) < BOUND
    eps = torch.randn(dist_r.mean.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(eps_seed))
    assert rel_inf(dist_m.sample(eps=eps), dist_r.mean + dist_r.std * eps) < BOUND
    return err


def test_tiny_encoder_matches_restatement():
    ref, m = _pair("tiny")
    _check_encoder(ref, m, seeded_pixels(2, 64, 48, seed=1, device=DEV))


@pytest.mark.parametrize("N,H,W", [(1, 512, 512), (2, 512, 512), (1, 576, 1024)])
def test_sd_vae_encoder_matches_restatement(N, H, W):
    ref, m = _pair("sd")
    x = seeded_pixels(N, H, W, seed=H + N, device=DEV)
    _check_encoder(ref, m, x)
    if N == 2:       # batch invariance: each image of the batch is bit-identical to the image encoded alone
        both = m.run(x)
        for i in range(N):
            assert torch.equal(both[i:i + 1], m.run(x[i:i + 1].clone()))


def test_graph_replay_is_bit_identical():
    _, m = _pair("tiny")
    x = seeded_pixels(2, 64, 64, seed=3, device=DEV)
    eager = m.run(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.run(x)                       # warm: the workspace of this size exists
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.run(x)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_pixel_dtypes(dt):
    ref, m = _pair("tiny")
    x = seeded_pixels(1, 32, 64, seed=4, device=DEV).to(dt)
    with torch.no_grad():
        want = ref.encode(x.float()).latent_dist.mode()
    assert rel_inf(m.run(x, out_dtype=torch.float32), want) < BOUND


def test_pipeline_helpers_match_restated_methods():
    import ctrl_adapter_amd as P
    ref, m = _pair("tiny")
    img = seeded_pixels(2, 64, 64, seed=6, device=DEV)
    with torch.no_grad():
        want = svd_encode_vae_image(ref, img, DEV, 2, True)
    got = P.encode_svd_image_latents(m, img, DEV, 2, True)
    assert got.shape == want.shape and rel_inf(got, want) < BOUND
    with torch.no_grad():
        want = i2vgen_prepare_image_latents(ref, img, DEV, 4, 2, True, generator=torch.Generator(device=DEV).manual_seed(3))
    got = P.prepare_i2vgen_image_latents(m, img, DEV, 4, 2, True, generator=torch.Generator(device=DEV).manual_seed(3))
    assert got.shape == want.shape == (8, 4, 4, 32, 32)
    assert rel_inf(got, want) < BOUND
    # the mirror's own distribution draws the same noise as the restatement's for the same generator
    s_m = m.encode(img).latent_dist.sample(torch.Generator(device=DEV).manual_seed(8))
    with torch.no_grad():
        s_r = ref.encode(img).latent_dist.sample(torch.Generator(device=DEV).manual_seed(8))
    assert rel_inf(s_m, s_r) < BOUND
