"""SDXL prompt encoding on the MI355X: the few-row GEMM (csrc/text_gemm.hip) against fp32 torch and across M, the wide row kernels,
OpenCLIP bigG at full shape (CLIPTextModelWithProjection) against the fp32 restatement (tests/clip_text_proj_ref.py, pinned to
transformers by tests/golden/clip_text_proj.pt), batch invariance, hidden_index / early exit, graph replays, encode_sdxl_prompt over
the mirrors, and the [2B, 77, 2048] states driving the SDXL-config ControlNetAdapter."""
import os
import sys

import pytest
import torch

from clip_text_proj_ref import BIGG, CLIPTextProjRef
from clip_text_ref import CLIPTextRef, SD15, seeded_ids
from test_gpu_text_encoder import rel_inf
from test_text_encoder_host import StubTokenizer
from test_text_encoder_proj_host import Pipe, pipeline_encode_prompt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EOS_REAL = 500
# bigG at 32 layers against the fp32 restatement: the issue's bound
BOUND = 1e-3


def _lib():
    from ctrl_adapter_amd import _lib
    return _lib


def text_gemm(x, W, b, act, res, out_dtype=torch.float32):
    L_ = _lib()
    M, K = x.shape
    N = W.shape[0]
    y = torch.full((M, N), float("nan"), dtype=out_dtype, device=DEV)
    ws = torch.empty(max(L_.lib().ctrl_text_gemm_ws_bytes(M, N, K) // 4, 1), dtype=torch.float32, device=DEV)
    L_.check(L_.lib().ctrl_op_text_gemm(L_.ptr(x), L_.ptr(W), L_.ptr(b), M, N, K, act, L_.ptr(res), L_.ptr(y), L_.dtype_code(out_dtype),
                                        L_.ptr(ws), ws.numel() * 4, L_.cur_stream()))
    torch.cuda.synchronize()
    return y


ACT = {0: lambda v: v, 2: lambda v: v * torch.sigmoid(1.702 * v), 3: lambda v: torch.nn.functional.gelu(v)}


@pytest.mark.parametrize("NK", [(1280, 5120), (5120, 1280), (3840, 1280), (768, 3072), (2304, 768)])
@pytest.mark.parametrize("act", [0, 2, 3])
def test_text_gemm_against_fp32_and_across_m(NK, act):
    N, K = NK
    g = torch.Generator().manual_seed(N + K + act)
    x = torch.randn(1232, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(N, generator=g) * 0.1
    res = torch.randn(1232, N, generator=g)
    xd, Wd, bd, rd = x.to(DEV), W.to(DEV), b.to(DEV), res.to(DEV)
    ys = {M: text_gemm(xd[:M].contiguous(), Wd, bd, act, rd[:M].contiguous()) for M in (1, 77, 154, 1232)}
    want = ACT[act](x.float() @ W.float().t() + b) + res
    e = rel_inf(ys[1232], want)
    print("text_gemm N %d K %d act %d: rel-inf %.2e" % (N, K, act, e))
    assert e <= 1e-5
    for M in (1, 77, 154):
        assert torch.equal(ys[M], ys[1232][:M]), "row bits depend on M = %d" % M
    y16 = text_gemm(xd[:154].contiguous(), Wd, bd, act, None, torch.float16)
    assert rel_inf(y16, ACT[act](x[:154].float() @ W.float().t() + b)) <= 1e-3


@pytest.mark.parametrize("C", [768, 1280, 2048])
def test_wide_row_kernels(C):
    L_ = _lib()
    N, L = 2, 77
    g = torch.Generator().manual_seed(C)
    V = 300
    tok, pos = torch.randn(V, C, generator=g), torch.randn(L, C, generator=g)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ids = seeded_ids(N, L, V, seed=C)
    x = torch.empty(N * L, C, device=DEV)
    y = torch.empty(N * L, C, dtype=torch.float16, device=DEV)
    d = [t.to(DEV) for t in (ids, tok, pos, gam, bet)]
    L_.check(L_.lib().ctrl_op_text_embed(L_.ptr(d[0]), L_.ptr(d[1]), L_.ptr(d[2]), V, N, L, C, L_.ptr(x), L_.ptr(d[3]), L_.ptr(d[4]),
                                         1e-5, L_.ptr(y), None, L_.cur_stream()))
    xr = (tok[ids] + pos[None]).reshape(N * L, C)
    yr = torch.nn.functional.layer_norm(xr, (C,), gam, bet, 1e-5)
    fy = torch.empty(N * L, C, device=DEV)
    pooled = torch.empty(N, C, device=DEV)
    L_.check(L_.lib().ctrl_op_text_final_ln(L_.ptr(x), 0, N * L, C, L_.ptr(d[3]), L_.ptr(d[4]), 1e-5, L_.ptr(fy), 0, L_.ptr(d[0]), L, 2,
                                            L_.ptr(pooled), L_.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), xr)
    assert rel_inf(y, yr) <= 1e-3
    assert rel_inf(fy, yr) <= 1e-5
    assert rel_inf(pooled, yr.view(N, L, C)[torch.arange(N), ids.argmax(-1)]) <= 1e-5


# ------------------------------------------------------------------------------------------ bigG at full shape
def _mirror(ref, cfg, gemm_form=None):
    import ctrl_adapter_amd as P
    m = P.CLIPTextModelWithProjection(**cfg, gemm_form=gemm_form)
    m.load_state_dict(ref.state_dict())
    return m.to(DEV)


@pytest.fixture(scope="module")
def bigg():
    torch.set_grad_enabled(False)
    from ctrl_adapter_amd.synthetic import seeded_init
    out = {}
    ref = seeded_init(CLIPTextProjRef(**BIGG).eval(), seed=47)
    for rule in ("argmax", "eos"):
        cfg = dict(BIGG, eos_token_id=2 if rule == "argmax" else EOS_REAL)
        r = CLIPTextProjRef(**cfg).eval()
        r.load_state_dict(ref.state_dict())
        out[rule] = (_mirror(r, cfg), r)
    out["form1"] = _mirror(out["argmax"][1], BIGG, gemm_form=1)
    return out


def _ids(N, rule, seed=7):
    return seeded_ids(N, 77, BIGG["vocab_size"], seed=seed, eos=None if rule == "argmax" else EOS_REAL)


_REF_CACHE = {}


def _ref_out(ref, rule, N):
    key = (rule, N)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = ref(_ids(N, rule), output_hidden_states=True)
    return _REF_CACHE[key]


@pytest.mark.parametrize("rule", ["argmax", "eos"])
@pytest.mark.parametrize("N", [1, 2, 4])
def test_bigg_against_restatement(bigg, rule, N):
    m, ref = bigg[rule]
    assert m.gemm_form == 0          # the default (the few-row GEMM loses at B = 16: profiles/sdxl_text_encoder_bench.txt)
    out = m(_ids(N, rule).to(DEV), output_hidden_states=True)
    want = _ref_out(ref, rule, N)
    errs = dict(text_embeds=rel_inf(out[0], want[0]), last=rel_inf(out[1], want[1]),
                penultimate=rel_inf(out.hidden_states[-2], want.hidden_states[-2]))
    print("bigG %s N=%d: %s" % (rule, N, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= BOUND, errs
    assert len(out.hidden_states) == 33 and out[0].shape == (N, 1280)


def test_bigg_few_row_gemm_form_within_bound(bigg):
    m1 = bigg["form1"]
    assert m1.gemm_form == 1
    ref = bigg["argmax"][1]
    out = m1(_ids(2, "argmax").to(DEV), output_hidden_states=True)
    want = _ref_out(ref, "argmax", 2)
    errs = (rel_inf(out[0], want[0]), rel_inf(out[1], want[1]), rel_inf(out.hidden_states[-2], want.hidden_states[-2]))
    print("bigG gemm_form 1: text_embeds %.2e last %.2e penultimate %.2e" % errs)
    assert max(errs) <= BOUND


@pytest.mark.parametrize("form", [0, 1])
def test_bigg_batch_invariance_and_hidden_index(bigg, form):
    from ctrl_adapter_amd.text_encoder import _forward_ext
    m = bigg["argmax"][0] if form == 0 else bigg["form1"]
    assert m.gemm_form == form
    ids16 = _ids(16, "argmax", seed=21).to(DEV)
    full = m(ids16, output_hidden_states=True)
    for n in (1, 2, 5):
        o = m(ids16[:n], output_hidden_states=True)
        assert torch.equal(o[0], full[0][:n]) and torch.equal(o[1], full[1][:n])
        assert torch.equal(o.hidden_states[-2], full.hidden_states[-2][:n])
    alone = m(ids16[3:4])
    assert torch.equal(alone[0], full[0][3:4]) and torch.equal(alone[1], full[1][3:4])
    # one state: with the tail, and alone (early exit after layer k); every path gives the bits of the all-states forward
    for k in (0, 5, 31, 32):
        _, _, emb, hk = _forward_ext(m, ids16[:2], embeds=True, hidden_index=k)
        _, _, _, hx = _forward_ext(m, ids16[:2], hidden_index=k)
        assert torch.equal(hk, full.hidden_states[k][:2]) and torch.equal(hx, hk), k
        assert torch.equal(emb, full[0][:2])


def test_bigg_graph_replays_dtypes_and_bad_ids(bigg):
    m, ref = bigg["argmax"]
    ids = _ids(2, "argmax", seed=5).to(DEV)
    eager = m(ids)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(ids)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(ids)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    want = ref(ids.cpu())
    for dt in (torch.float16, torch.bfloat16):
        mh = _mirror(ref, BIGG).to(dt)
        o = mh(ids)
        assert o[0].dtype == dt and o[1].dtype == dt
        bound = 4e-3 if dt == torch.float16 else 2e-2
        assert rel_inf(o[0], want[0]) <= bound and rel_inf(o[1], want[1]) <= bound
        del mh
    bad = ids.clone()
    bad[0, 3] = BIGG["vocab_size"]
    with pytest.raises(ValueError, match="vocabulary"):
        m(bad)
    with pytest.raises(ValueError, match="vocabulary"):
        m(bad.cpu())


# ------------------------------------------------------------------------------------------ encode_sdxl_prompt + the adapter
@pytest.fixture(scope="module")
def sdxl_towers(bigg):
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    ref_l = seeded_init(CLIPTextRef(**SD15).eval(), seed=49)
    ml = P.CLIPTextModel(**SD15)
    ml.load_state_dict(ref_l.state_dict())
    mg, ref_g = bigg["argmax"]

    class RefL(torch.nn.Module):        # the CLIP-L restatement with transformers' output object
        def __init__(self):
            super().__init__()
            self.r = ref_l
            self.config = ref_l.config

        @property
        def dtype(self):
            return torch.float32

        def forward(self, ids, output_hidden_states=False):
            from clip_text_proj_ref import _Out
            last, pooled, hs = self.r(ids, output_hidden_states=True)
            return _Out(last, pooled, hs)
    return [ml.to(DEV), mg], [RefL(), ref_g]


@pytest.mark.parametrize("clip_skip", [None, 1])
def test_encode_sdxl_prompt_on_the_mirrors(sdxl_towers, clip_skip):
    import ctrl_adapter_amd as P
    mirrors, refs = sdxl_towers
    toks = [StubTokenizer(SD15["vocab_size"]), StubTokenizer(BIGG["vocab_size"])]
    kw = dict(prompt=["a cat on a mat", "a dog"], negative_prompt=["blurry", ""], num_images_per_prompt=2, clip_skip=clip_skip)
    got = P.encode_sdxl_prompt(toks, mirrors, device=DEV, force_zeros_for_empty_prompt=False, **kw)
    want = pipeline_encode_prompt(Pipe(toks, mirrors, False), device=DEV, **kw)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    ref = pipeline_encode_prompt(Pipe(toks, refs, False), device="cpu", **kw)
    errs = [rel_inf(a, b) for a, b in zip(got, ref)]
    print("encode_sdxl_prompt (clip_skip %s) vs restatement: %s" % (clip_skip, ", ".join("%.2e" % e for e in errs)))
    assert got[0].shape == (4, 77, 2048) and max(errs) <= BOUND


def test_sdxl_states_drive_the_adapter(sdxl_towers):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import cases
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    mirrors, refs = sdxl_towers
    toks = [StubTokenizer(SD15["vocab_size"]), StubTokenizer(BIGG["vocab_size"])]
    kw = dict(prompt=["a cat on a mat", "a dog"], negative_prompt=["blurry", "dark"])
    pe, npe, _, _ = P.encode_sdxl_prompt(toks, mirrors, device=DEV, force_zeros_for_empty_prompt=False, **kw)
    rpe, rnpe, _, _ = pipeline_encode_prompt(Pipe(toks, refs, False), device="cpu", **kw)
    ehs, ehs_ref = torch.cat([npe, pe]), torch.cat([rnpe, rpe])
    assert ehs.shape == (4, 77, 2048)
    inp = cases.controlnet_inputs(N=4, hs=16)
    cn = seeded_init(P.ControlNetModel(**cases.CONTROLNET_KW), seed=11).to(DEV)
    ad = seeded_init(P.ControlNetAdapter(**cases.ADAPTER_SDXL), seed=22).to(DEV)
    down, _ = cn(inp["sample"].half().to(DEV), inp["timestep"].to(DEV), inp["encoder_hidden_states"].half().to(DEV),
                 inp["controlnet_cond"].half().to(DEV), return_dict=False)
    out, _ = ad(down, num_frames=1, timestep=torch.tensor(499.0), encoder_hidden_states=ehs.half())
    out_ref, _ = ad(down, num_frames=1, timestep=torch.tensor(499.0), encoder_hidden_states=ehs_ref.half().to(DEV))
    torch.cuda.synchronize()
    worst = max(rel_inf(a, b) for a, b in zip(out, out_ref) if a is not None)
    e_in = rel_inf(ehs, ehs_ref)
    # the adapter carries the states' error into its outputs: measured 6.3e-4 in, 1.15e-3 out (1.8x) on the first run; the bound
    # is 2.5x the error of the states it was fed, and never below the suite's 1e-3
    bound = max(BOUND, 2.5 * e_in)
    print("SDXL adapter on the HIP states vs the restatement's: worst rel-inf %.2e (states %.2e, bound %.2e)" % (worst, e_in, bound))
    assert worst <= bound
