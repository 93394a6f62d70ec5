"""The C-ABI library loads and exports every symbol include/ctrl_hip.h declares (no compute calls: CPU box)."""
import ctypes
import os
import re

from helpers import ROOT


def test_library_exports_every_declared_symbol():
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ctrl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)        # drop comments
    declared = set(re.findall(r"\b(ctrl_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 30
    for name in sorted(declared):
        assert hasattr(lib, name), "libctrlhip.so does not export %s" % name
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    # the test ABI of the implicit GEMM: the pinned form, the split-K sizing queries (tests/test_gpu_igemm_forms.py) and the form
    # selector (tests/test_igemm_select_host.py)
    assert {"ctrl_op_igemm_pinned", "ctrl_igemm_splitk_factor", "ctrl_igemm_splitk_ws_bytes", "ctrl_igemm_splitk_ticket_words",
            "ctrl_igemm_select"} <= declared
    # the grouped attention launch, reached outside a plan only through this entry (tests/test_gpu_attn_forms.py)
    assert "ctrl_op_flash_attn_group" in declared
    # the test ABI of the norm and streaming kernels (tests/norm_forms.py, tests/test_gpu_norm_forms.py, tests/test_gpu_stream_forms.py)
    assert {"ctrl_op_gn_stats_group", "ctrl_op_gn_apply_group", "ctrl_op_gn_fused_group", "ctrl_gn_launch_shape", "ctrl_op_layernorm_group",
            "ctrl_op_layernorm_add", "ctrl_op_add_rowvec_clip", "ctrl_op_upsample2x_nhwc", "ctrl_op_fill_zero_group",
            "ctrl_op_linear_small_group", "ctrl_op_frameidx_sincos"} <= declared
    # the test ABI of the fused feed-forward's grouped launch and of the fp32 stem convolutions (tests/ffn_forms.py,
    # tests/test_gpu_ffn_forms.py, tests/smallconv_forms.py, tests/test_gpu_smallconv_forms.py)
    assert {"ctrl_op_ffn_group", "ctrl_op_conv3x3_direct_f32", "ctrl_op_conv3x3_rows_f32"} <= declared
    # the test ABI of the CLIP towers' kernels that only a plan reached (tests/tower_forms.py, tests/test_gpu_tower_forms.py)
    assert {"ctrl_op_text_gemm_finish", "ctrl_op_text_proj", "ctrl_op_text_store", "ctrl_op_vision_vt", "ctrl_op_text_final_ln_ext"} <= declared
    # the test ABI of the helper kernels: the packers with the caller's fp16 range flag, the transpose with an image map and the three
    # per-pixel kernels only a plan reached (tests/helper_forms.py, tests/test_gpu_helper_forms.py)
    assert {"ctrl_op_pack_conv_w_ovf", "ctrl_op_pack_conv_w_dup_ovf", "ctrl_op_pack_conv_w_phase_ovf", "ctrl_op_pack_linear_w_ovf",
            "ctrl_op_nhwc_to_nchw_map", "ctrl_op_unet_conv_out", "ctrl_op_i2v_frames", "ctrl_op_vae_conv_in"} <= declared
    # the test ABI of the VAE and UNet shell kernels: the skip join with a split mirror, which only a plan reached (tests/shell_forms.py,
    # tests/test_gpu_shell_forms.py)
    assert "ctrl_op_unet_skip_join_split" in declared
    assert lib.ctrl_abi_version() == _lib.ABI_VERSION == 11


def test_struct_sizes_match_header():
    """ctypes mirrors must have the C layout (sizes computed from the header's field order by gcc)."""
    import subprocess
    import tempfile
    from ctrl_adapter_amd import _lib
    src = '#include "ctrl_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ctrl_igemm_seg), sizeof(ctrl_igemm_desc), sizeof(ctrl_attn_desc), sizeof(ctrl_tattn_desc), sizeof(ctrl_tensor_ref), sizeof(ctrl_controlnet_config), sizeof(ctrl_adapter_config), sizeof(ctrl_clip_comm), sizeof(ctrl_ffn_desc), sizeof(ctrl_gn_desc), sizeof(ctrl_ln_desc), sizeof(ctrl_small_lin));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    got = [ctypes.sizeof(c) for c in (_lib.IGemmSeg, _lib.IGemmDesc, _lib.AttnDesc, _lib.TAttnDesc, _lib.TensorRef,
                                     _lib.ControlNetConfig, _lib.AdapterConfig, _lib.ClipComm, _lib.FfnDesc, _lib.GnDesc, _lib.LnDesc, _lib.SmallLin)]
    assert [int(v) for v in out] == got, (out, got)


def test_every_tile_walk_order_is_a_bijection():
    """csrc/tile_order.h decides which output tile a workgroup of the implicit GEMM computes; any order is correct as long as
    it is a bijection of the grid, so that is what is proved here (host integer code, no GPU): every mode x group width over
    the grid shapes of the path (incl. the ragged ones that fall back to the legacy walk), and the locality property the
    grouped walk exists for."""
    from ctrl_adapter_amd import _lib
    lib = _lib.lib()
    tm, tn = ctypes.c_int(), ctypes.c_int()

    def walk(ntm, ntn, mode, group):
        out = []
        for bid in range(ntm * ntn):
            assert lib.ctrl_igemm_tile_of(bid, ntm, ntn, mode, group, ctypes.byref(tm), ctypes.byref(tn)) == 0
            out.append((tm.value, tn.value))
        return out

    grids = [(512, 32), (128, 16), (32, 20), (8, 40), (8, 8), (64, 4), (512, 1), (1, 1), (3, 5), (7, 16), (24, 3), (40, 13)]
    for ntm, ntn in grids:
        want = {(m, n) for m in range(ntm) for n in range(ntn)}
        for mode in (0, 1, 2):
            for group in (0, 1, 2, 3, 5, 8, 12, 16, 64):
                got = walk(ntm, ntn, mode, group)
                assert len(set(got)) == len(got) == ntm * ntn and set(got) == want, (ntm, ntn, mode, group)
    # legacy == the M-major list cut into 8 contiguous ranges, one per XCD (workgroup b runs on XCD b % 8)
    got = walk(16, 4, 0, 0)
    assert [got[b] for b in range(0, 64, 8)] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]
    assert got[1] == (2, 0) and got[7] == (14, 0)
    # xcd_m, groups of 2: an XCD sweeps its own 2 activation panels against weight panels {0, 1}, then against {2, 3}
    got = walk(16, 4, 1, 2)
    assert [got[b] for b in range(0, 64, 8)] == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (0, 3), (1, 2), (1, 3)]
    assert {got[b][0] for b in range(3, 128 // 2, 8)} == {6, 7}
    # xcd_n: XCD x owns weight panels [x * ntn / 8, (x + 1) * ntn / 8) and every activation panel
    got = walk(4, 16, 2, 0)
    assert {got[b][1] for b in range(5, 64, 8)} == {10, 11} and {got[b][0] for b in range(5, 64, 8)} == {0, 1, 2, 3}
    assert lib.ctrl_igemm_tile_of(64, 8, 8, 0, 0, ctypes.byref(tm), ctypes.byref(tn)) == 1      # out of range: refused
    for spec, rc in ((b"legacy", 0), (b"m,16", 0), (b"n,0", 0), (b"sideways", 1), (b"auto", 0)):
        assert lib.ctrl_igemm_set_order(spec) == rc, spec
