"""SDXL's backbone UNet, host side (no GPU): the parameter inventory against the restatement's diffusers keys (tests/unet_sdxl_ref.py)
for the five test configs; at the real SDXL config, from the inventory alone, the published parameter total and the nine skips; the C
struct's size and the new symbols; persistence and a config dict with every key of SDXL-base's unet/config.json; the forward
signature; every refusal; the mid residual given as 0 / 0.0 / None; and the restatement's two up blocks held bit for bit against the
same forward written out by hand from oracle/blocks.py calls on shared weights."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import unet_sdxl_ref as R
from helpers import ROOT
from oracle import blocks as O

CFGS = sorted(R.CONFIGS)
SDXL_PARAMETERS = 2567463684         # the published size of SDXL-base's UNet


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def _c_cfg(cfg):
    from ctrl_adapter_amd.unet_2d_condition import unet2d_config
    return unet2d_config(4, 4, cfg["down_block_types"], cfg["up_block_types"], cfg["block_out_channels"], cfg["layers_per_block"],
                         cfg["transformer_layers_per_block"], cfg["attention_head_dim"], cfg["cross_attention_dim"],
                         cfg["addition_time_embed_dim"], cfg["projection_class_embeddings_input_dim"], 1e-5)


@pytest.mark.parametrize("name", CFGS)
def test_param_spec_equals_diffusers_keys(name):
    from ctrl_adapter_amd.unet_2d_condition import unet2d_spec
    cfg = R.CONFIGS[name]
    with torch.device("meta"):
        ref = R.UNetSdxlRef(**cfg)
    want = _shapes(ref.state_dict())
    spec = unet2d_spec(_c_cfg(cfg))
    assert len(spec) == len(dict(spec)) and dict(spec) == want
    boc, lpb = cfg["block_out_channels"], cfg["layers_per_block"]
    sd = dict(spec)
    assert sd["up_blocks.0.resnets.0.conv1.weight"] == (boc[-1], boc[-1] + boc[-1], 3, 3)
    assert sd["up_blocks.%d.resnets.%d.conv1.weight" % (len(boc) - 1, lpb)] == (boc[0], boc[0] + boc[0], 3, 3)
    assert sd["up_blocks.%d.resnets.0.conv_shortcut.weight" % (len(boc) - 1)] == (boc[0], boc[1] + boc[0], 1, 1)
    assert sd["conv_in.weight"] == (boc[0], 4, 3, 3) and sd["conv_out.weight"] == (4, boc[0], 3, 3)
    assert sd["add_embedding.linear_1.weight"] == (4 * boc[0], cfg["projection_class_embeddings_input_dim"])
    assert sd["mid_block.attentions.0.proj_in.weight"] == (boc[-1], boc[-1])             # linear projections: 2-D keys
    assert sd["mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (boc[-1], cfg["cross_attention_dim"])
    # the depth per level, reversed in the up path: the first up block mirrors the LAST level
    depth = cfg["transformer_layers_per_block"]
    for blk, d in (("mid_block.attentions.0", depth[-1]), ("up_blocks.0.attentions.%d" % lpb, depth[-1]),
                   ("down_blocks.1.attentions.0", depth[1])):
        assert blk + ".transformer_blocks.%d.norm1.weight" % (d - 1) in sd and blk + ".transformer_blocks.%d.norm1.weight" % d not in sd
    assert not any(k.startswith("down_blocks.0.attentions") or k.startswith("up_blocks.%d.attentions" % (len(boc) - 1)) for k in sd)


def test_module_state_dict_is_the_inventory():
    import ctrl_adapter_amd as P
    for name in ("TWO", "LPB1"):
        with torch.device("meta"):
            ref = R.UNetSdxlRef(**R.CONFIGS[name])
        m = P.UNet2DConditionModel(**R.CONFIGS[name])
        assert _shapes(m.state_dict()) == _shapes(ref.state_dict())
        assert m.dtype == torch.float32 and m.device.type == "cpu"


def test_real_sdxl_inventory_has_the_published_parameter_total_and_nine_skips():
    """from the inventory alone: no weights are allocated"""
    from ctrl_adapter_amd.unet_2d_condition import unet2d_spec
    spec = unet2d_spec(_c_cfg(R.SDXL))
    total = 0
    for _, shape in spec:
        n = 1
        for d in shape:
            n *= d
        total += n
    assert total == SDXL_PARAMETERS, total
    with torch.device("meta"):
        ref = R.UNetSdxlRef(**R.SDXL)
    assert dict(spec) == _shapes(ref.state_dict())
    assert sum(p.numel() for p in ref.parameters()) == SDXL_PARAMETERS
    shapes, mid = R.skip_shapes(R.SDXL, 128, 128)
    assert len(shapes) == 9 and mid == (1280, 32, 32)
    # the 70 cross-attentions of a forward: 2 x 2 (level 1) + 2 x 10 (level 2) + 10 (mid) + 3 x 10 + 3 x 2 (up)
    assert sum(1 for k, _ in spec if k.endswith("attn2.to_q.weight")) == 70
    # the module's own bookkeeping of the skips, without building it: the same rule, from a small config
    import ctrl_adapter_amd as P
    m = P.UNet2DConditionModel(**R.THREE)
    assert len(m._skips) == 9 and [c for c, _ in m._skips] == [s[0] for s in R.skip_shapes(R.THREE, 16, 16)[0]]
    assert [f for _, f in m._skips] == [1, 1, 1, 2, 2, 2, 4, 4, 4] and m._mid == (256, 4)


def test_config_struct_size_matches_the_header_and_symbols_resolve(tmp_path):
    from ctrl_adapter_amd import _lib
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "ctrl_hip.h"\nint main(void) { printf("%zu\\n", sizeof(ctrl_unet2d_config)); return 0; }\n')
    exe = tmp_path / "size"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.call(["sh", "-c", "command -v %s >/dev/null" % c]) == 0), None)
    assert cc is not None, "no C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == ctypes.sizeof(_lib.UNet2DConfig)
    lib = _lib.lib()
    for name in ("ctrl_unet2d_param_count", "ctrl_unet2d_param_spec", "ctrl_unet2d_create", "ctrl_unet2d_destroy", "ctrl_unet2d_selection",
                 "ctrl_unet2d_set_text_cache", "ctrl_unet2d_forward", "ctrl_unet2d_workspace_bytes", "ctrl_op_unet_text_time"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 11 and lib.ctrl_abi_version() == 11


# every key of SDXL-base's unet/config.json (diffusers 0.19), with the widths of LPB1
def _sdxl_config_json(cfg):
    return dict(act_fn="silu", addition_embed_type="text_time", addition_embed_type_num_heads=64,
                addition_time_embed_dim=cfg["addition_time_embed_dim"], attention_head_dim=list(cfg["attention_head_dim"]),
                block_out_channels=list(cfg["block_out_channels"]), center_input_sample=False, class_embed_type=None,
                class_embeddings_concat=False, conv_in_kernel=3, conv_out_kernel=3, cross_attention_dim=cfg["cross_attention_dim"],
                cross_attention_norm=None, down_block_types=list(cfg["down_block_types"]), downsample_padding=1, dual_cross_attention=False,
                encoder_hid_dim=None, encoder_hid_dim_type=None, flip_sin_to_cos=True, freq_shift=0, in_channels=4,
                layers_per_block=cfg["layers_per_block"], mid_block_only_cross_attention=None, mid_block_scale_factor=1,
                mid_block_type="UNetMidBlock2DCrossAttn", norm_eps=1e-05, norm_num_groups=32, num_attention_heads=None, num_class_embeds=None,
                only_cross_attention=False, out_channels=4,
                projection_class_embeddings_input_dim=cfg["projection_class_embeddings_input_dim"], resnet_out_scale_factor=1.0,
                resnet_skip_time_act=False, resnet_time_scale_shift="default", sample_size=128, time_cond_proj_dim=None,
                time_embedding_act_fn=None, time_embedding_dim=None, time_embedding_type="positional", timestep_post_act=None,
                transformer_layers_per_block=list(cfg["transformer_layers_per_block"]), up_block_types=list(cfg["up_block_types"]),
                upcast_attention=None, use_linear_projection=True)


def test_a_config_dict_loads_and_save_pretrained_round_trips(tmp_path):
    import ctrl_adapter_amd as P
    ref = R.seeded_unet(R.LPB1, 11)
    m = P.UNet2DConditionModel(**_sdxl_config_json(R.LPB1))
    m.load_state_dict(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    m.save_pretrained(str(tmp_path))
    m2 = P.UNet2DConditionModel.from_pretrained(str(tmp_path), torch_dtype=torch.float16)
    assert m2.dtype == torch.float16 and m2.device.type == "cpu"
    assert m2.config.sample_size == 128 and tuple(m2.config.block_out_channels) == R.LPB1["block_out_channels"]
    assert set(m2.state_dict()) == set(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m2.state_dict()[k].float(), v), k
    # the defaults are SDXL-base's
    sig = inspect.signature(P.UNet2DConditionModel.__init__).parameters
    for k, v in _sdxl_config_json(R.SDXL).items():
        if k != "sample_size":
            d = sig[k].default
            assert (list(d) if isinstance(d, tuple) else d) == v, k


def test_forward_signature_is_diffusers():
    import ctrl_adapter_amd as P
    names = list(inspect.signature(P.UNet2DConditionModel.forward).parameters)
    assert names == ["self", "sample", "timestep", "encoder_hidden_states", "class_labels", "timestep_cond", "attention_mask",
                     "cross_attention_kwargs", "added_cond_kwargs", "down_block_additional_residuals", "mid_block_additional_residual",
                     "down_intrablock_additional_residuals", "encoder_attention_mask", "return_dict"]
    assert list(inspect.signature(R.UNetSdxlRef.forward).parameters)[:len(names)] == names
    out = P.UNet2DConditionOutput(torch.zeros(1))
    assert isinstance(out, tuple) and out[0] is out.sample and len(out) == 1
    assert hasattr(P.UNet2DConditionModel, "cache_text") and P.UNet2DConditionModel.cache_text is False


_REFUSED = r"^UNet2DConditionModel \(libctrlhip\): "


@pytest.mark.parametrize("key,value", [
    ("center_input_sample", True), ("flip_sin_to_cos", False), ("freq_shift", 1), ("mid_block_type", "UNetMidBlock2DSimpleCrossAttn"),
    ("only_cross_attention", True), ("downsample_padding", 0), ("mid_block_scale_factor", 2), ("dropout", 0.1), ("act_fn", "gelu"),
    ("norm_num_groups", 16), ("encoder_hid_dim", 64), ("encoder_hid_dim_type", "text_proj"), ("dual_cross_attention", True),
    ("use_linear_projection", False), ("class_embed_type", "timestep"), ("addition_embed_type", "text"), ("addition_embed_type", None),
    ("num_class_embeds", 10), ("upcast_attention", True), ("resnet_time_scale_shift", "scale_shift"), ("resnet_skip_time_act", True),
    ("resnet_out_scale_factor", 2.0), ("time_embedding_type", "fourier"), ("time_embedding_dim", 64), ("time_embedding_act_fn", "silu"),
    ("timestep_post_act", "silu"), ("time_cond_proj_dim", 8), ("conv_in_kernel", 5), ("conv_out_kernel", 5),
    ("class_embeddings_concat", True), ("mid_block_only_cross_attention", True), ("cross_attention_norm", "layer_norm"),
    ("addition_embed_type_num_heads", 32), ("attention_type", "gated"), ("reverse_transformer_layers_per_block", [[1], [1]])])
def test_any_other_config_value_is_refused(key, value):
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError, match=_REFUSED + ".*unsupported configuration.*" + key):
        P.UNet2DConditionModel(**dict(R.LPB1, **{key: value}))


def test_constructor_refusals():
    import ctrl_adapter_amd as P
    U = P.UNet2DConditionModel
    with pytest.raises(ValueError, match=_REFUSED + ".*block type"):
        U(**dict(R.TWO, down_block_types=("DownBlock2D", "AttnDownBlock2D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*block type"):
        U(**dict(R.TWO, up_block_types=("CrossAttnUpBlock2D", "UpBlock3D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*mirror"):
        U(**dict(R.TWO, up_block_types=("UpBlock2D", "CrossAttnUpBlock2D")))
    with pytest.raises(ValueError, match=_REFUSED + ".*must be 64"):
        U(**dict(R.TWO, attention_head_dim=(1, 4)))                           # 128 // 4 = 32 at the attention level (and the mid block)
    with pytest.raises(ValueError, match=_REFUSED + ".*must be 64"):
        U(**dict(R.THREE, attention_head_dim=(1, 2, 8)))
    with pytest.raises(ValueError, match=_REFUSED + ".*must be 64"):
        U(**dict(R.TWO, num_attention_heads=(1, 4)))                          # num_attention_heads wins over attention_head_dim
    with pytest.raises(ValueError, match=_REFUSED + ".*same number"):
        U(**dict(R.TWO, transformer_layers_per_block=(1, 2, 3)))
    U(**dict(R.TWO, attention_head_dim=(7, 2)))                               # level 0 does not attend: its head count is not read
    assert U(**dict(R.TWO, attention_head_dim=(1, 4), num_attention_heads=(1, 2)))._cfg.num_attention_heads[1] == 2


def _args(m, B=2, h=16, w=16, keys=77, **over):
    cfg = R.TWO
    kw = dict(sample=torch.zeros(B, 4, h, w), encoder_hidden_states=torch.zeros(B, keys, cfg["cross_attention_dim"]), class_labels=None,
              timestep_cond=None, attention_mask=None, cross_attention_kwargs=None,
              added_cond_kwargs=dict(text_embeds=torch.zeros(B, R.text_dim(cfg)), time_ids=torch.zeros(B, 6)),
              mid_block_additional_residual=None, down_intrablock_additional_residuals=None, encoder_attention_mask=None)
    kw.update(over)
    return m._check_args(**kw)


def test_forward_refusals_run_before_any_launch():
    import ctrl_adapter_amd as P
    m = P.UNet2DConditionModel(**R.TWO)
    z = torch.zeros(1)
    _args(m)
    _args(m, cross_attention_kwargs={})
    _args(m, keys=8)
    _args(m, h=8, w=24)
    for bad in (dict(h=12), dict(w=20), dict(h=4)):
        with pytest.raises(ValueError, match=_REFUSED + ".*multiples of 8"):
            _args(m, **bad)
    for name in ("class_labels", "timestep_cond", "attention_mask", "encoder_attention_mask", "down_intrablock_additional_residuals"):
        with pytest.raises(ValueError, match=_REFUSED + ".*`%s`" % name):
            _args(m, **{name: z})
    with pytest.raises(ValueError, match=_REFUSED + ".*cross_attention_kwargs"):
        _args(m, cross_attention_kwargs={"scale": 0.5})
    with pytest.raises(ValueError, match=_REFUSED + ".*added_cond_kwargs"):
        _args(m, added_cond_kwargs=None)
    ok = dict(text_embeds=torch.zeros(2, 64), time_ids=torch.zeros(2, 6))
    with pytest.raises(ValueError, match=_REFUSED + ".*image_embeds"):
        _args(m, added_cond_kwargs=dict(ok, image_embeds=z))
    with pytest.raises(ValueError, match=_REFUSED + ".*unsupported key"):
        _args(m, added_cond_kwargs=dict(ok, aesthetic_score=z))
    with pytest.raises(ValueError, match=_REFUSED + ".*must hold"):
        _args(m, added_cond_kwargs=dict(text_embeds=ok["text_embeds"]))
    with pytest.raises(ValueError, match=_REFUSED + ".*projection_class_embeddings_input_dim"):
        _args(m, added_cond_kwargs=dict(ok, time_ids=torch.zeros(2, 5)))
    with pytest.raises(ValueError, match=_REFUSED + ".*projection_class_embeddings_input_dim"):
        _args(m, added_cond_kwargs=dict(ok, text_embeds=torch.zeros(2, 96)))
    _args(m, added_cond_kwargs=dict(text_embeds=torch.zeros(2, 96), time_ids=torch.zeros(2, 5)))       # the generic n_ids rule: 96 + 5 * 32
    with pytest.raises(ValueError, match=_REFUSED + ".*encoder_hidden_states"):
        _args(m, encoder_hidden_states=torch.zeros(2, 77, 64))
    with pytest.raises(ValueError, match=_REFUSED + ".*sample must be"):
        _args(m, sample=torch.zeros(2, 8, 16, 16))
    # the full forward refuses the same way, before the device check
    with pytest.raises(ValueError, match=_REFUSED + ".*`class_labels`"):
        m(torch.zeros(2, 4, 16, 16), 5.0, torch.zeros(2, 77, 128), class_labels=z, added_cond_kwargs=ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 4, 16, 16), 5.0, torch.zeros(2, 77, 128), added_cond_kwargs=ok, mid_block_additional_residual=0)


def test_mid_residual_zero_number_is_no_residual_and_other_numbers_are_refused():
    import ctrl_adapter_amd as P
    m = P.UNet2DConditionModel(**R.TWO)
    for v in (0, 0.0, None):
        assert _args(m, mid_block_additional_residual=v)[2] is None
    t = torch.zeros(2, 128, 8, 8)
    assert _args(m, mid_block_additional_residual=t)[2] is t
    for v in (1, 0.5, -1, True, "0"):
        with pytest.raises(ValueError, match=_REFUSED + ".*mid_block_additional_residual"):
            _args(m, mid_block_additional_residual=v)


# ------------------------------------------------------------------------------------------------ the restatement against the oracle's blocks
def _by_hand_transformer(t, x, ehs):
    """Transformer2DModel(use_linear_projection) from the oracle's leaves: GroupNorm, Linear, BasicTransformerBlocks, Linear, + input"""
    b, c, h, w = x.shape
    tok = F.linear(F.group_norm(x, 32, t.norm.weight, t.norm.bias, 1e-6).permute(0, 2, 3, 1).reshape(b, h * w, c), t.proj_in.weight, t.proj_in.bias)
    for src in t.transformer_blocks:
        blk = O.BasicTransformerBlock(c, src.attn1.heads, c // src.attn1.heads, ehs.shape[-1]).eval()
        blk.load_state_dict(src.state_dict())
        tok = blk(tok, encoder_hidden_states=ehs)
    tok = F.linear(tok, t.proj_out.weight, t.proj_out.bias)
    return tok.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous() + x


def _by_hand_up(blk, hidden, skips, temb, ehs, cin_first, cout):
    for i, res in enumerate(blk.resnets):
        cat = torch.cat([hidden, skips[-1 - i]], dim=1)
        plain = O.ResnetBlock2D(in_channels=cat.shape[1], out_channels=cout, temb_channels=temb.shape[1], eps=1e-5).eval()
        plain.load_state_dict(res.state_dict())
        hidden = plain(cat, temb)
        if blk.has_cross_attention:
            hidden = _by_hand_transformer(blk.attentions[i], hidden, ehs)
    up = blk.upsamplers[0]
    return F.conv2d(O.Upsample2D(cout)(hidden), up.conv.weight, up.conv.bias, padding=1)


@pytest.mark.parametrize("cross", [True, False], ids=["CrossAttnUpBlock2D", "UpBlock2D"])
def test_restated_up_blocks_are_the_oracles_leaves_bit_for_bit(cross):
    from ctrl_adapter_amd.synthetic import seeded_init
    cin, prev, cout, temb_c, layers = 64, 256, 128, 96, 3
    if cross:
        blk = R.CrossAttnUpBlock2D(cin, prev, cout, temb_c, layers, 1e-5, True, 2, 48, 2)
    else:
        blk = R.UpBlock2D(cin, prev, cout, temb_c, layers, 1e-5, True)
    blk = seeded_init(blk, seed=5).eval()
    assert [r.conv1.weight.shape[1] for r in blk.resnets] == [prev + cout, cout + cout, cout + cin]
    g = torch.Generator().manual_seed(1)
    hidden, temb, ehs = torch.randn(2, prev, 4, 6, generator=g), torch.randn(2, temb_c, generator=g), torch.randn(2, 5, 48, generator=g)
    skips = (torch.randn(2, cin, 4, 6, generator=g), torch.randn(2, cout, 4, 6, generator=g), torch.randn(2, cout, 4, 6, generator=g))
    with torch.no_grad():
        got = blk(hidden, skips, temb=temb, encoder_hidden_states=ehs)
        want = _by_hand_up(blk, hidden, skips, temb, ehs, prev, cout)
    assert got.shape == (2, cout, 8, 12) and torch.equal(got, want)
    if cross:       # the transformers are there, two layers deep
        assert len(blk.attentions) == layers and len(blk.attentions[0].transformer_blocks) == 2
        with torch.no_grad():
            assert not torch.equal(blk(hidden, skips, temb=temb, encoder_hidden_states=2 * ehs), got)


def test_restated_text_time_embedding_puts_the_text_first():
    ref = R.seeded_unet(R.LPB1, 3)
    g = torch.Generator().manual_seed(2)
    text, ids = torch.randn(2, 64, generator=g), torch.tensor([[512.0, 768.0, 0.0, 16.0, 512.0, 768.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    with torch.no_grad():
        got = ref.text_time_embedding(text, ids, torch.float32)
        sin = torch.cat([O.get_timestep_embedding(ids[b], 32, flip_sin_to_cos=True, downscale_freq_shift=0).reshape(1, -1) for b in range(2)])
        want = ref.add_embedding(torch.cat([text, sin], dim=-1))
    assert torch.equal(got, want)


def test_restated_forward_zero_residuals_equal_none_and_a_short_list_pairs_from_the_front():
    ref = R.seeded_unet(R.LPB1, 21)
    B, h, w = 1, 8, 8
    inp = R.make_inputs(R.LPB1, B, h, w, keys=8, seed=4, residuals=True, res_dtype=torch.float32)
    plain = {k: v for k, v in inp.items() if "residual" not in k}
    with torch.no_grad():
        base, stages = ref(**plain, return_stages=True)
        zeros = dict(plain, down_block_additional_residuals=[torch.zeros_like(r) for r in inp["down_block_additional_residuals"]],
                     mid_block_additional_residual=0)
        assert torch.equal(ref(**zeros).sample, base)
        full = ref(**inp).sample
        assert not torch.equal(full, base) and base.shape == (B, 4, h, w)
        short = dict(inp, down_block_additional_residuals=inp["down_block_additional_residuals"][:-2])
        padded = dict(inp, down_block_additional_residuals=inp["down_block_additional_residuals"][:-2]
                      + [torch.zeros_like(r) for r in inp["down_block_additional_residuals"][-2:]])
        assert torch.equal(ref(**short).sample, ref(**padded).sample)
        assert torch.equal(ref(**dict(plain, timestep=37.0), return_dict=False)[0], base)
    shapes, mid = R.skip_shapes(R.LPB1, h, w)
    assert len(shapes) == 4                       # conv_in, one layer, the down-sampler, one layer
    assert [tuple(s.shape[1:]) for s in stages["skips"]] == shapes and tuple(stages["mid"].shape[1:]) == mid
