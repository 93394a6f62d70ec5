"""I2VGen-XL's backbone UNet, host side (no GPU): the parameter inventory against the restatement's keys (tests/unet_i2vgen_ref.py) for
every config -- the real one on the meta device --, spot keys, the skip count, the C struct's size, the new symbols, the forward
signature, every refusal, persistence, and the restatement held against itself: TemporalConvLayerRef and TransformerTemporalRef against
the same arithmetic written out with plain F.group_norm / F.conv3d / F.scaled_dot_product_attention on shared weights, to fp32
round-off; the 4-D and 5-D residual layouts agree."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import unet_i2vgen_ref as R
from helpers import ROOT

CFGS = sorted(R.CONFIGS)
# the real config's parameter total, computed from the inventory (DESIGN.md section 7 quotes it; no published figure is at hand to pin it to)
I2VGEN_PARAMS = 1420469224


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("name", CFGS)
def test_param_spec_equals_the_restatements_keys(name):
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.unet_i2vgen_xl import unet_i2v_spec
    cfg = R.CONFIGS[name]
    with torch.device("meta"):
        ref = R.I2VGenUNetRef(**cfg)
        m = P.I2VGenXLUNet(**cfg)
    want = _shapes(ref.state_dict())
    spec = unet_i2v_spec(m._cfg)
    assert len(spec) == len(dict(spec)) and dict(spec) == want
    sd = _shapes(m.state_dict())
    assert sd == want
    boc, cross = cfg["block_out_channels"], cfg["cross_attention_dim"]
    C0 = boc[0]
    assert sd["down_blocks.0.temp_convs.0.conv1.2.weight"] == (C0, C0, 3, 1, 1)
    assert sd["down_blocks.0.temp_convs.0.conv2.3.weight"] == (C0, C0, 3, 1, 1) and sd["down_blocks.0.temp_convs.0.conv4.0.weight"] == (C0,)
    assert sd["down_blocks.0.temp_attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (C0, C0)          # double self-attention
    assert sd["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (C0, cross)
    assert sd["down_blocks.0.attentions.0.proj_in.weight"] == (C0, C0)                                       # linear projections
    assert sd["transformer_in.proj_in.weight"] == (512, C0) and sd["transformer_in.proj_out.weight"] == (C0, 512)
    assert sd["transformer_in.transformer_blocks.0.ff.net.0.proj.weight"] == (4096, 512)
    assert sd["conv_in.weight"] == (C0, 8, 3, 3) and sd["conv_out.weight"] == (4, C0, 3, 3)
    assert sd["image_latents_temporal_encoder.ff.net.0.proj.weight"] == (16, 4)
    assert sd["image_latents_temporal_encoder.attn1.to_q.weight"] == (8, 4) and "image_latents_temporal_encoder.attn1.to_q.bias" not in sd
    assert sd["image_latents_proj_in.4.weight"] == (4, 16, 3, 3) and sd["image_latents_context_embedding.5.weight"] == (cross, 64, 3, 3)
    assert sd["context_embedding.2.weight"] == (4 * cross, 4 * C0) and sd["fps_embedding.0.weight"] == (4 * C0, C0)
    assert sd["up_blocks.0.resnets.0.conv1.weight"] == (boc[-1], 2 * boc[-1], 3, 3)
    assert sd["mid_block.temp_convs.1.conv4.3.bias"] == (boc[-1],) and "mid_block.attentions.1.norm.weight" not in sd
    n_skips = 1 + sum(cfg["layers_per_block"] + (1 if i + 1 < len(boc) else 0) for i in range(len(boc)))
    assert len(m._skips) == n_skips == len(R.skip_shapes(cfg, 1, 1, 64, 64)[0])
    if name == "I2VGEN":
        assert n_skips == 12
        assert sum(torch.Size(s).numel() for s in want.values()) == I2VGEN_PARAMS


def test_config_struct_size_matches_the_header_and_symbols_resolve(tmp_path):
    from ctrl_adapter_amd import _lib
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "ctrl_hip.h"\nint main(void) { printf("%zu\\n", sizeof(ctrl_unet_i2v_config)); return 0; }\n')
    exe = tmp_path / "size"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.call(["sh", "-c", "command -v %s >/dev/null" % c]) == 0), None)
    assert cc is not None, "no C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == ctypes.sizeof(_lib.UNetI2VConfig)
    lib = _lib.lib()
    for name in ("ctrl_unet_i2v_param_count", "ctrl_unet_i2v_param_spec", "ctrl_unet_i2v_create", "ctrl_unet_i2v_destroy", "ctrl_unet_i2v_selection",
                 "ctrl_unet_i2v_set_cond_cache", "ctrl_unet_i2v_forward", "ctrl_unet_i2v_workspace_bytes", "ctrl_op_i2v_latent_encoder",
                 "ctrl_op_adaptive_avgpool_nhwc"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 11 and lib.ctrl_abi_version() == 11


def test_forward_signature_is_the_references():
    import ctrl_adapter_amd as P
    names = list(inspect.signature(P.I2VGenXLUNet.forward).parameters)
    assert names == ["self", "sample", "timestep", "fps", "image_latents", "image_embeddings", "encoder_hidden_states", "timestep_cond",
                     "cross_attention_kwargs", "down_block_additional_residuals", "mid_block_additional_residual", "return_dict"]
    assert list(inspect.signature(R.I2VGenUNetRef.forward).parameters)[:len(names)] == names
    ctor = list(inspect.signature(P.I2VGenXLUNet.__init__).parameters)
    assert ctor == ["self", "sample_size", "in_channels", "out_channels", "down_block_types", "up_block_types", "block_out_channels",
                    "layers_per_block", "norm_num_groups", "cross_attention_dim", "attention_head_dim", "num_attention_heads"]
    assert list(inspect.signature(R.I2VGenUNetRef.__init__).parameters) == ctor
    out = P.UNet3DConditionOutput(torch.zeros(1))
    assert isinstance(out, tuple) and out[0] is out.sample and len(out) == 1
    m = P.I2VGenXLUNet(**R.NARROW)
    assert m.dtype == torch.float32 and m.device.type == "cpu" and m.config.in_channels == 4 and m.config.attention_head_dim == 64
    assert m.cache_condition is False and m.selection is None
    real = P.I2VGenXLUNet.__init__.__defaults__
    assert (320, 640, 1280, 1280) in real and 1024 in real           # the defaults are the real config


_REFUSED = r"^I2VGenXLUNet \(libctrlhip\): "


def test_constructor_refusals():
    import ctrl_adapter_amd as P
    U = P.I2VGenXLUNet
    with pytest.raises(ValueError, match=_REFUSED + ".*in_channels"):
        U(**dict(R.NARROW, in_channels=8))
    with pytest.raises(ValueError, match=_REFUSED + ".*norm_num_groups"):
        U(**R.NARROW, norm_num_groups=16)
    with pytest.raises(ValueError, match=_REFUSED + ".*attention_head_dim"):
        U(**R.NARROW, attention_head_dim=32)
    with pytest.raises(ValueError, match=_REFUSED + ".*attention_head_dim"):
        U(**R.NARROW, attention_head_dim=(64, 32))
    with pytest.raises(ValueError, match=_REFUSED + ".*block type.*down_block_types"):
        U(**dict(R.NARROW, down_block_types=("CrossAttnDownBlock2D", "DownBlock3D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*block type"):
        U(**dict(R.NARROW, up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlock3D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*mirror"):
        U(**dict(R.NARROW, up_block_types=("CrossAttnUpBlock3D", "UpBlock3D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*same number"):
        U(**dict(R.NARROW, block_out_channels=(64, 128, 128)))
    U(**R.NARROW, attention_head_dim=(64, 64), num_attention_heads=8)          # num_attention_heads is ignored, as in the reference


class _OnGpu:
    """a module that says it lives on the GPU: forward's input checks run (and refuse) before anything touches a device"""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        type(self.m).device = property(lambda s: torch.device("cuda", 0))
        return self.m

    def __exit__(self, *a):
        del type(self.m).device


def test_forward_refusals_run_before_any_launch():
    import ctrl_adapter_amd as P

    class U(P.I2VGenXLUNet):       # (a subclass, so the patched `device` does not leak into the package's class)
        pass

    class FakeCuda(torch.Tensor):
        """a CPU tensor that reports itself on cuda:0"""
        is_cuda = property(lambda s: True)
        device = property(lambda s: torch.device("cuda", 0))

    def fake(*shape):
        return torch.zeros(*shape).as_subclass(FakeCuda)

    with _OnGpu(U(**R.THREE)) as m:
        fps, lat, emb, ehs = fake(2), fake(2, 4, 3, 16, 16), fake(2, 128), fake(2, 77, 128)
        ok = fake(2, 4, 3, 16, 16)
        with pytest.raises(ValueError, match=_REFUSED + ".*timestep_cond"):
            m(ok, 5.0, fps, lat, emb, ehs, timestep_cond=fake(2, 8))
        with pytest.raises(ValueError, match=_REFUSED + ".*cross_attention_kwargs"):
            m(ok, 5.0, fps, lat, emb, ehs, cross_attention_kwargs={"scale": 0.5})
        with pytest.raises(ValueError, match=_REFUSED + ".*image_embeddings"):
            m(ok, 5.0, fps, lat, None, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*encoder_hidden_states"):
            m(ok, 5.0, fps, lat, emb, None)
        with pytest.raises(ValueError, match=_REFUSED + ".*multiples of 4"):
            m(fake(2, 4, 3, 18, 16), 5.0, fps, fake(2, 4, 3, 18, 16), emb, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*multiples of 4"):
            m(fake(2, 4, 3, 16, 2), 5.0, fps, fake(2, 4, 3, 16, 2), emb, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*at most 32 frames"):
            m(fake(2, 4, 33, 16, 16), 5.0, fps, fake(2, 4, 33, 16, 16), emb, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*sample must be"):
            m(fake(2, 8, 3, 16, 16), 5.0, fps, lat, emb, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*image_latents"):
            m(ok, 5.0, fps, fake(2, 4, 1, 16, 16), emb, ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*image_embeddings"):
            m(ok, 5.0, fps, lat, fake(2, 64), ehs)
        with pytest.raises(ValueError, match=_REFUSED + ".*encoder_hidden_states"):
            m(ok, 5.0, fps, lat, emb, fake(2, 77, 64))
        assert m._check_args(ok, lat, emb, ehs, None, {}) == (2, 3, 16, 16)          # an empty cross_attention_kwargs passes
    m = P.I2VGenXLUNet(**R.NARROW)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 4, 2, 8, 8), 5.0, torch.zeros(1), torch.zeros(1, 4, 2, 8, 8), torch.zeros(1, 128), torch.zeros(1, 5, 128))


def test_state_dict_and_save_pretrained_round_trip(tmp_path):
    import ctrl_adapter_amd as P
    ref = R.seeded_unet(R.NARROW, 11)
    m = P.I2VGenXLUNet(**R.NARROW, sample_size=32)
    sd = ref.state_dict()
    # a [C, C, 1, 1] projection weight (the transformers' projections as 1x1 convolutions) is accepted and flattened
    conv_style = dict(sd)
    k = "down_blocks.0.attentions.0.proj_in.weight"
    conv_style[k] = sd[k][:, :, None, None]
    m.load_state_dict(conv_style)
    for key, v in sd.items():
        assert torch.equal(m.state_dict()[key], v), key
    m.save_pretrained(str(tmp_path))
    m2 = P.I2VGenXLUNet.from_pretrained(str(tmp_path), torch_dtype=torch.float16)
    assert m2.dtype == torch.float16 and m2.device.type == "cpu"
    assert m2.config.sample_size == 32 and tuple(m2.config.block_out_channels) == R.NARROW["block_out_channels"]
    assert tuple(m2.config.down_block_types) == R.NARROW["down_block_types"]
    assert set(m2.state_dict()) == set(sd)
    for key, v in sd.items():
        assert torch.equal(m2.state_dict()[key].float(), v), key
    assert m2.half() is m2 and m2.to(torch.float32).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ the restatement against itself
def _close(a, b, what):
    err = (a - b).abs().max().item() / b.abs().max().item()
    assert err < 2e-6, (what, err)          # fp32 round-off of two orders of the same arithmetic


def test_temporal_conv_layer_ref_is_four_groupnorm_silu_conv3d_plus_identity():
    from ctrl_adapter_amd.synthetic import seeded_init
    C, B, nf, h, w = 64, 2, 3, 4, 5
    blk = seeded_init(R.TemporalConvLayerRef(C), seed=5).eval()
    sd = blk.state_dict()
    assert sorted(sd) == sorted("conv%d.%d.%s" % (i, j, p) for i in (1, 2, 3, 4) for j in ((0, 2) if i == 1 else (0, 3)) for p in ("weight", "bias"))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * nf, C, h, w, generator=g)
    with torch.no_grad():
        got = blk(x, num_frames=nf)
        y = x.reshape(B, nf, C, h, w).permute(0, 2, 1, 3, 4)                  # b c f h w
        z = y
        for i in (1, 2, 3, 4):
            conv = "conv%d.%d" % (i, 2 if i == 1 else 3)
            z = F.group_norm(z, 32, sd["conv%d.0.weight" % i], sd["conv%d.0.bias" % i], eps=1e-5)      # statistics span the frames
            z = F.conv3d(F.silu(z), sd[conv + ".weight"], sd[conv + ".bias"], padding=(1, 0, 0))
        want = (y + z).permute(0, 2, 1, 3, 4).reshape(B * nf, C, h, w)
    _close(got, want, "temporal conv")
    # the statistics are the clip's, not the frame's: normalising frame by frame gives something else
    with torch.no_grad():
        per_frame = F.group_norm(x, 32, sd["conv1.0.weight"], sd["conv1.0.bias"], eps=1e-5)
        clip = F.group_norm(y, 32, sd["conv1.0.weight"], sd["conv1.0.bias"], eps=1e-5).permute(0, 2, 1, 3, 4).reshape(B * nf, C, h, w)
    assert (per_frame - clip).abs().max() > 1e-3
    with torch.no_grad():                    # one frame: the (3,1,1) convolutions see their zero padding only
        assert blk(x[:2], num_frames=1).shape == (2, C, h, w)


def test_transformer_temporal_ref_is_two_self_attentions_over_the_frames():
    from ctrl_adapter_amd.synthetic import seeded_init
    C, heads, B, nf, h, w = 64, 2, 2, 3, 2, 3
    inner = heads * 64
    t = seeded_init(R.TransformerTemporalRef(heads, 64, C), seed=6).eval()
    sd = t.state_dict()
    assert sd["transformer_blocks.0.attn2.to_k.weight"].shape == (inner, inner)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B * nf, C, h, w, generator=g)

    def attn(pre, tok):
        q, k, v = (F.linear(tok, sd[pre + ".to_%s.weight" % n]).view(tok.shape[0], nf, heads, 64).transpose(1, 2) for n in "qkv")
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(tok.shape[0], nf, inner)
        return F.linear(o, sd[pre + ".to_out.0.weight"], sd[pre + ".to_out.0.bias"])

    def ln(name, tok):
        return F.layer_norm(tok, (inner,), sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)

    with torch.no_grad():
        got = t(x, num_frames=nf)
        y = x.reshape(B, nf, C, h, w).permute(0, 2, 1, 3, 4)
        y = F.group_norm(y, 32, sd["norm.weight"], sd["norm.bias"], eps=1e-6)
        tok = y.permute(0, 3, 4, 2, 1).reshape(B * h * w, nf, C)                  # one sequence of F tokens per pixel
        tok = F.linear(tok, sd["proj_in.weight"], sd["proj_in.bias"])
        b = "transformer_blocks.0"
        tok = tok + attn(b + ".attn1", ln(b + ".norm1", tok))
        tok = tok + attn(b + ".attn2", ln(b + ".norm2", tok))
        hid, gate = F.linear(ln(b + ".norm3", tok), sd[b + ".ff.net.0.proj.weight"], sd[b + ".ff.net.0.proj.bias"]).chunk(2, dim=-1)
        tok = tok + F.linear(hid * F.gelu(gate), sd[b + ".ff.net.2.weight"], sd[b + ".ff.net.2.bias"])
        tok = F.linear(tok, sd["proj_out.weight"], sd["proj_out.bias"])
        want = tok.reshape(B, h, w, nf, C).permute(0, 3, 4, 1, 2).reshape(B * nf, C, h, w) + x
    _close(got, want, "temporal transformer")
    # the token order (b h w, f, c) is the frame-major row order (b f, h w, c) read with a stride: no permutation is needed
    rows = x.permute(0, 2, 3, 1).reshape(B, nf, h * w, C)
    assert torch.equal(rows.permute(0, 2, 1, 3).reshape(B * h * w, nf, C), x.reshape(B, nf, C, h, w).permute(0, 3, 4, 1, 2).reshape(B * h * w, nf, C))


def test_restated_forward_zero_residuals_equal_none_and_layouts_agree():
    ref = R.seeded_unet(R.NARROW, 21)
    B, nf, h, w = 1, 2, 8, 8
    inp = R.seeded_inputs(R.NARROW, B, nf, h, w, seed=4, residuals="4d", text_len=5, res_dtype=torch.float32)
    inp5 = R.seeded_inputs(R.NARROW, B, nf, h, w, seed=4, residuals="5d", text_len=5, res_dtype=torch.float32)
    assert inp5["down_block_additional_residuals"][0].shape == (B, 64, nf, h, w)
    plain = {k: v for k, v in inp.items() if "residual" not in k}
    with torch.no_grad():
        base, stages = ref(**plain, return_stages=True)
        zeros = dict(plain, down_block_additional_residuals=[torch.zeros_like(r) for r in inp["down_block_additional_residuals"]],
                     mid_block_additional_residual=torch.zeros_like(inp["mid_block_additional_residual"]))
        assert torch.equal(ref(**zeros).sample, base)
        with4 = ref(**inp).sample
        assert torch.equal(ref(**inp5).sample, with4)
        assert not torch.equal(with4, base)
        assert base.shape == (B, 4, nf, h, w)
        # the zero-initialised convolutions carry signal: switching one temporal conv's conv4 off moves the output
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.state_dict()["down_blocks.0.temp_convs.0.conv4.3.weight"].zero_()
        ref.state_dict()["down_blocks.0.temp_convs.0.conv4.3.bias"].zero_()
        assert (ref(**plain).sample - base).abs().max() > 1e-3
        ref.load_state_dict(sd)
        # a timestep as a Python number gives what the [B] tensor of the same value gives
        assert torch.equal(ref(**dict(plain, timestep=37.0), return_dict=False)[0], base)
    shapes, mid = R.skip_shapes(R.NARROW, B, nf, h, w)
    assert [tuple(s.shape[1:]) for s in stages["skips"]] == shapes and tuple(stages["mid"].shape[1:]) == mid
