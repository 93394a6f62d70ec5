"""CLIP text encoder on the MI355X: the new kernels (causal attention, quick_gelu epilogue) against fp32 torch, the whole encoder
against the fp32 restatement (tests/clip_text_ref.py, pinned to transformers by tests/golden/clip_text.pt), batch invariance,
graph replays, encode_controlnet_prompt end to end and the text states driving the HIP ControlNet."""
import ctypes as C

import pytest
import torch

from clip_text_ref import CLIPTextRef, SD15, seeded_ids
from test_text_encoder_host import StubTokenizer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EOS_REAL = 500


def rel_inf(a, b):
    """max|a - b| / max|b|, the parity metric of the suite"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _lib():
    from ctrl_adapter_amd import _lib
    return _lib


def seeded_pair(cfg, seed=41, **kw):
    """the HIP mirror on the GPU and the fp32 restatement on the CPU, same seeded weights"""
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    ref = seeded_init(CLIPTextRef(**cfg).eval(), seed=seed, **kw)
    m = P.CLIPTextModel(**cfg)
    m.load_state_dict(ref.state_dict())
    return m.to(DEV), ref


@pytest.fixture(scope="module")
def sd15():
    torch.set_grad_enabled(False)
    return {rule: seeded_pair(dict(SD15, eos_token_id=2 if rule == "argmax" else EOS_REAL)) for rule in ("argmax", "eos")}


def _ids(N, rule, seed=7):
    return seeded_ids(N, 77, SD15["vocab_size"], seed=seed, eos=None if rule == "argmax" else EOS_REAL)


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("L", [1, 2, 16, 76, 77])
@pytest.mark.parametrize("N", [1, 2, 16])          # x 12 heads: 12, 24, 192 (prompt, head) pairs
def test_text_attention_op(L, N):
    L_ = _lib()
    heads, D = 12, 64
    Cn = heads * D
    g = torch.Generator().manual_seed(L * 100 + N)
    qkv = torch.randn(N * L, 3 * Cn, generator=g).half()
    out = torch.full((N * L, Cn), float("nan"), dtype=torch.float16, device=DEV)
    qd = qkv.to(DEV)
    L_.check(L_.lib().ctrl_op_text_attn(L_.ptr(qd), 3 * Cn, L_.ptr(out), Cn, N, L, heads, 0.125, L_.cur_stream()))
    torch.cuda.synchronize()
    x = qkv.float().view(N, L, 3, heads, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    want = (s.softmax(-1) @ v).transpose(1, 2).reshape(N * L, Cn)
    assert torch.isfinite(out).all()
    assert rel_inf(out, want) <= 2e-3


def test_quick_gelu_epilogue():
    L_ = _lib()
    M, K, N = 154, 768, 3072
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).half().to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half().to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(DEV)
    outs = {}
    for act in (0, 1, 2):
        y = torch.empty(M, N, dtype=torch.float16, device=DEV)
        d = L_.IGemmDesc()
        d.A, d.lda, d.mode, d.Cin, d.taps = x.data_ptr(), K, 0, K, 1
        d.W, d.M, d.Nout, d.Ktot, d.bias, d.scale, d.act = w.data_ptr(), M, N, K, b.data_ptr(), 1.0, act
        d.nseg = 1
        d.seg[0].out, d.seg[0].ld, d.seg[0].col_begin, d.seg[0].ncols, d.seg[0].fmt, d.seg[0].dtype, d.seg[0].L = y.data_ptr(), N, 0, N, 0, L_.F16, 1
        L_.check(L_.lib().ctrl_op_igemm(C.byref(d), L_.cur_stream()))
        outs[act] = y
    torch.cuda.synchronize()
    h = x.float() @ w.float().t() + b
    assert rel_inf(outs[0], h) <= 1e-3
    assert rel_inf(outs[1], h * torch.sigmoid(h)) <= 1e-3
    assert rel_inf(outs[2], h * torch.sigmoid(1.702 * h)) <= 1e-3


# ------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("rule", ["argmax", "eos"])
@pytest.mark.parametrize("N", [1, 2, 16])
def test_encoder_sd15_against_restatement(sd15, rule, N):
    m, ref = sd15[rule]
    ids = _ids(N, rule, seed=N)
    out = m(ids.to(DEV), output_hidden_states=True)
    torch.cuda.synchronize()
    last, pooled, hs = ref(ids, output_hidden_states=True)
    e_last, e_pool = rel_inf(out[0], last), rel_inf(out[1], pooled)
    print("N=%d %s: last %.2e pooled %.2e" % (N, rule, e_last, e_pool))
    assert e_last <= 1e-3 and e_pool <= 1e-3
    assert len(out[-1]) == 13
    for k in (0, 6, 11, 12):
        assert rel_inf(out[-1][k], hs[k]) <= 1e-3, k
    for clip_skip in (1, 2):
        got = m.text_model.final_layer_norm(out[-1][-(clip_skip + 1)])
        want = ref.text_model.final_layer_norm(hs[-(clip_skip + 1)])
        assert rel_inf(got, want) <= 1e-3, clip_skip


def test_encoder_out_of_vocab_ids_raise(sd15):
    m, _ = sd15["argmax"]
    ids = _ids(1, "argmax")
    ids[0, 3] = SD15["vocab_size"] + 5
    with pytest.raises(ValueError, match="vocabulary"):
        m(ids)                           # host ids: checked before upload
    with pytest.raises(ValueError, match="vocabulary"):
        m(ids.to(DEV))                   # device ids: clamped by the kernel, flagged, raised
    out = m(_ids(1, "argmax").to(DEV))   # the flag was reset
    assert torch.isfinite(out[0]).all()


@pytest.mark.parametrize("dtype,bound", [(torch.float16, 2e-3), (torch.bfloat16, 8e-3)])
def test_encoder_half_outputs(sd15, dtype, bound):
    m32, ref = sd15["argmax"]
    m = type(m32)(**dict(m32.config))
    m.load_state_dict(m32.state_dict())
    m = m.to(DEV, dtype)
    r = type(ref)(**SD15)
    r.load_state_dict({k: v.to(dtype).float() for k, v in ref.state_dict().items()})    # the weights as the cast model holds them
    ids = _ids(2, "argmax", seed=5)
    out = m(ids.to(DEV))
    torch.cuda.synchronize()
    last, pooled = r(ids)[:2]
    assert out[0].dtype == dtype and out[1].dtype == dtype
    e = max(rel_inf(out[0], last), rel_inf(out[1], pooled))
    print("%s outputs: rel-inf %.2e (bound %.0e)" % (dtype, e, bound))
    assert e <= bound


def test_encoder_batch_invariance(sd15):
    m, _ = sd15["argmax"]
    ids = _ids(16, "argmax", seed=21).to(DEV)
    full = m(ids, output_hidden_states=True)
    for i in (0, 5, 15):
        one = m(ids[i:i + 1], output_hidden_states=True)
        assert torch.equal(one[0][0], full[0][i]) and torch.equal(one[1][0], full[1][i]), i
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one[-1], full[-1])), i
    pair = m(ids[3:5])
    assert torch.equal(pair[0], full[0][3:5])


def test_encoder_eager_and_graph_replays_bit_identical(sd15):
    m, _ = sd15["argmax"]
    ids = _ids(4, "argmax", seed=31).to(DEV)
    a = m(ids)
    b = m(ids)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(ids)                            # workspace in place before the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(ids)
    for _ in range(50):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1])


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("clip_skip", [None, 1])
def test_encode_controlnet_prompt_mirror_vs_restatement(sd15, clip_skip):
    from ctrl_adapter_amd import encode_controlnet_prompt
    m, ref = sd15["argmax"]
    tok = StubTokenizer(SD15["vocab_size"])
    args = (["a cat on a mat", "a dog"], 2, True)
    got = encode_controlnet_prompt(tok, m, args[0], DEV, *args[1:], negative_prompt=["blurry", ""], clip_skip=clip_skip)
    want = encode_controlnet_prompt(tok, ref, args[0], "cpu", *args[1:], negative_prompt=["blurry", ""], clip_skip=clip_skip)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.device.type == "cuda"
        assert rel_inf(a, b) <= 1e-3


def test_text_states_drive_the_controlnet(sd15):
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import cases
    import ctrl_adapter_amd as P
    from oracle.init import seeded_init
    from oracle.controlnet import ControlNetOracle
    m, ref = sd15["argmax"]
    ids = _ids(2, "argmax", seed=41)
    ehs = m(ids.to(DEV))[0]
    ehs_ref = ref(ids)[0]
    inp = cases.controlnet_inputs(N=2, hs=8)
    cn = seeded_init(P.ControlNetModel(**cases.CONTROLNET_KW), seed=11).to(DEV)
    down, mid = cn(inp["sample"].half().to(DEV), inp["timestep"].to(DEV), ehs.half(), inp["controlnet_cond"].half().to(DEV),
                   return_dict=False)
    torch.cuda.synchronize()
    oc = seeded_init(ControlNetOracle(**cases.CONTROLNET_KW).eval(), seed=11)
    rd, rm = oc(inp["sample"], inp["timestep"], ehs_ref, inp["controlnet_cond"])
    worst = max(rel_inf(a, b) for a, b in list(zip(down, rd)) + [(mid, rm)])
    print("ControlNet on the encoder's states: worst rel-inf %.2e" % worst)
    assert worst <= 1e-3


def test_weight_gain_two_sweep():
    """gain 2 (std * sqrt(fan_in) = 2 for every weight matrix): the fp16-operand error grows as in the issue's emulation (2.8e-3 last,
    2.2e-3 pooled); bound 5e-3"""
    m, ref = seeded_pair(SD15, seed=43, gain=2.0)
    ids = _ids(4, "argmax", seed=8)
    out = m(ids.to(DEV))
    torch.cuda.synchronize()
    last, pooled = ref(ids)[:2]
    e_last, e_pool = rel_inf(out[0], last), rel_inf(out[1], pooled)
    print("gain 2: last %.2e pooled %.2e (bound 5e-3)" % (e_last, e_pool))
    assert e_last <= 5e-3 and e_pool <= 5e-3
