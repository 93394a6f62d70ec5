"""ctypes binding of libctrlhip.so (the C ABI declared in include/ctrl_hip.h).

There is no fallback: if the shared library is missing or fails to load, importing the product path
raises.  PyTorch is used only for device memory and streams; every tensor crosses this boundary as a
raw device pointer.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libctrlhip.so")

F32, F16, BF16 = 0, 1, 2


class IGemmSeg(C.Structure):
    _fields_ = [("out", C.c_void_p), ("ld", C.c_int64), ("col_begin", C.c_int32), ("ncols", C.c_int32),
                ("fmt", C.c_int32), ("dtype", C.c_int32), ("L", C.c_int32), ("pad_", C.c_int32), ("img_map", C.c_void_p)]


class IGemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("mode", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32),
                ("Hin", C.c_int32), ("Win", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32),
                ("stride", C.c_int32), ("up", C.c_int32), ("F", C.c_int32), ("HW", C.c_int32), ("t_pad", C.c_int32),
                ("W", C.c_void_p), ("M", C.c_int32), ("Nout", C.c_int32), ("Ktot", C.c_int32), ("tap_origin", C.c_int32),
                ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("rowvec_ld", C.c_int32), ("rows_per_img", C.c_int32),
                ("res", C.c_void_p), ("ldres", C.c_int64), ("scale", C.c_float), ("geglu", C.c_int32),
                ("nseg", C.c_int32), ("act", C.c_int32), ("res_f32", C.c_int32), ("a_split", C.c_int32),
                ("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_int64), ("splitk_tickets", C.c_void_p),
                ("out16", C.c_void_p), ("ld16", C.c_int64),
                ("blend_mix", C.c_void_p), ("blend_x", C.c_void_p), ("ld_blend", C.c_int64), ("blend_f32", C.c_int32), ("out16_lo_off", C.c_int32), ("scale2", C.c_float), ("scale2_from", C.c_int32),
                ("res_up", C.c_int32), ("scale2_to", C.c_int32),
                ("seg", IGemmSeg * 3), ("nonfinite", C.c_void_p)]


class FfnDesc(C.Structure):
    _fields_ = [("X", C.c_void_p), ("ldx", C.c_int64), ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2p", C.c_void_p), ("out", IGemmDesc)]


class AttnDesc(C.Structure):
    _fields_ = [("Q", C.c_void_p), ("ldq", C.c_int64), ("K", C.c_void_p), ("ldk", C.c_int64),
                ("Vt", C.c_void_p), ("Lkpad", C.c_int32), ("kvB", C.c_int32),
                ("O", C.c_void_p), ("ldo", C.c_int64),
                ("B", C.c_int32), ("heads", C.c_int32), ("D", C.c_int32), ("Lq", C.c_int32), ("Lk", C.c_int32),
                ("scale", C.c_float), ("k_prescaled", C.c_int32), ("pad0_", C.c_int32)]


class TAttnDesc(C.Structure):
    _fields_ = [("Q", C.c_void_p), ("ld", C.c_int64), ("O", C.c_void_p), ("ldo", C.c_int64),
                ("Bc", C.c_int32), ("F", C.c_int32), ("HW", C.c_int32), ("heads", C.c_int32),
                ("scale", C.c_float), ("Fq", C.c_int32), ("KV", C.c_void_p), ("ldkv", C.c_int64),
                ("Fl", C.c_int32), ("pad0_", C.c_int32)]


class GnDesc(C.Structure):
    """ctrl_gn_desc: one GroupNorm problem with every argument of the op layer"""
    _fields_ = [("x", C.c_void_p), ("x_dtype", C.c_int32), ("silu", C.c_int32),
                ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("y", C.c_void_p),
                ("imgs", C.c_int32), ("rows_per_img", C.c_int32), ("C", C.c_int32), ("G", C.c_int32),
                ("eps", C.c_float), ("lo_off", C.c_int32),
                ("ldx", C.c_int64), ("ldy", C.c_int64), ("stat_rows", C.c_int64), ("y_img_rows", C.c_int64), ("y_row0", C.c_int64)]


class LnDesc(C.Structure):
    """ctrl_ln_desc: one LayerNorm problem (optionally with the added per-image vector)"""
    _fields_ = [("x", C.c_void_p), ("x_dtype", C.c_int32), ("M", C.c_int32), ("ldx", C.c_int64),
                ("addv", C.c_void_p), ("ldv", C.c_int64), ("rows_per_img", C.c_int32), ("vmod", C.c_int32), ("xsum", C.c_void_p),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("y", C.c_void_p), ("ldy", C.c_int64),
                ("C", C.c_int32), ("eps", C.c_float)]


class SmallLin(C.Structure):
    """ctrl_small_lin: one problem of ctrl_op_linear_small_group"""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("w", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("in_silu", C.c_int32), ("out_silu", C.c_int32), ("pad0_", C.c_int32)]


class TensorRef(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int32), ("ndim", C.c_int32),
                ("shape", C.c_int64 * 6)]


class ControlNetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("conditioning_channels", C.c_int32),
                ("block_out_channels", C.c_int32 * 4), ("down_block_has_attn", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("num_attention_heads", C.c_int32),
                ("cross_attention_dim", C.c_int32), ("cond_embed_channels", C.c_int32 * 4),
                ("norm_eps", C.c_float)]


class AdapterConfig(C.Structure):
    _fields_ = [("backbone_sdxl", C.c_int32), ("num_blocks", C.c_int32), ("num_adapters_per_location", C.c_int32),
                ("cross_attention_dim", C.c_int32),
                ("add_spatial_resnet", C.c_int32), ("add_temporal_resnet", C.c_int32),
                ("add_spatial_transformer", C.c_int32), ("add_temporal_transformer", C.c_int32),
                ("loc_A", C.c_int32), ("loc_B", C.c_int32), ("loc_C", C.c_int32), ("loc_D", C.c_int32),
                ("loc_M", C.c_int32)]


class TextEncoderConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32), ("max_position_embeddings", C.c_int32),
                ("eos_token_id", C.c_int32), ("layer_norm_eps", C.c_float)]


class TextEncoderExt(C.Structure):
    _fields_ = [("hidden_act", C.c_int32), ("projection_dim", C.c_int32), ("gemm_form", C.c_int32), ("reserved", C.c_int32)]


class VisionEncoderConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32), ("projection_dim", C.c_int32),
                ("hidden_act", C.c_int32), ("layer_norm_eps", C.c_float), ("gemm_form", C.c_int32)]


class VaeEncoderConfig(C.Structure):
    _fields_ = [("num_levels", C.c_int32), ("block_out_channels", C.c_int32 * 4), ("layers_per_block", C.c_int32),
                ("latent_channels", C.c_int32), ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float)]


VAE_MODE, VAE_SAMPLE, VAE_MOMENTS = 0, 1, 2      # output kinds of ctrl_vae_encoder_forward / ctrl_op_vae_posterior


class VaeDecoderConfig(C.Structure):
    _fields_ = [("num_levels", C.c_int32), ("block_out_channels", C.c_int32 * 4), ("layers_per_block", C.c_int32),
                ("latent_channels", C.c_int32), ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float), ("out_channels", C.c_int32)]


class UNetSTConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_levels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("transformer_layers_per_block", C.c_int32), ("num_attention_heads", C.c_int32 * 4),
                ("cross_attention_dim", C.c_int32), ("level_has_attn", C.c_int32 * 4), ("addition_time_embed_dim", C.c_int32),
                ("projection_class_embeddings_input_dim", C.c_int32)]


class UNet2DConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_levels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("transformer_layers_per_block", C.c_int32 * 4), ("num_attention_heads", C.c_int32 * 4),
                ("cross_attention_dim", C.c_int32), ("level_has_attn", C.c_int32 * 4), ("addition_time_embed_dim", C.c_int32),
                ("projection_class_embeddings_input_dim", C.c_int32), ("norm_eps", C.c_float)]


class UNetI2VConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_levels", C.c_int32), ("block_out_channels", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("cross_attention_dim", C.c_int32), ("level_has_attn", C.c_int32 * 4)]


class SamplerDesc(C.Structure):
    """ctrl_sampler_desc: the latents, the model output and the model inputs of one sampler launch"""
    _fields_ = [("x", C.c_void_p), ("prev", C.c_void_p), ("model_out", C.c_void_p), ("g", C.c_void_p), ("unet_in", C.c_void_p),
                ("concat", C.c_void_p), ("cn_in", C.c_void_p),
                ("x_dtype", C.c_int32), ("prev_dtype", C.c_int32), ("mo_dtype", C.c_int32), ("unet_dtype", C.c_int32),
                ("concat_dtype", C.c_int32), ("cn_dtype", C.c_int32),
                ("outer", C.c_int32), ("C", C.c_int32), ("inner", C.c_int32), ("C2", C.c_int32), ("R", C.c_int32),
                ("cn_frames", C.c_int32), ("g_count", C.c_int32), ("g_inner", C.c_int32), ("g_scalar", C.c_float), ("pad0_", C.c_int32)]


MERGE_SLOTS = 13      # CTRL_MERGE_SLOTS


class MergeSlot(C.Structure):
    _fields_ = [("inp", C.c_void_p * 8), ("out", C.c_void_p), ("elems", C.c_int64), ("row", C.c_int32), ("pad0_", C.c_int32)]


SAMPLER_ROW = 8       # CTRL_SAMPLER_ROW: c_in, A, B, t_model, t_aux0, t_aux1, 0, 0


VAE_DEC_SAMPLE, VAE_DEC_UNIT, VAE_DEC_U8 = 0, 1, 2      # epilogues of ctrl_vae_decoder_forward / ctrl_op_vae_dec_tail


class HedConfig(C.Structure):
    _fields_ = [("trunk_scale", C.c_float), ("reserved", C.c_int32), ("ws_cap_bytes", C.c_int64)]


class PidiConfig(C.Structure):
    _fields_ = [("frames_per_group", C.c_int32), ("reserved", C.c_int32), ("ws_cap_bytes", C.c_int64)]


class LineartConfig(C.Structure):
    _fields_ = [("frames_per_group", C.c_int32), ("has_coarse", C.c_int32), ("ws_cap_bytes", C.c_int64)]


U8_NHWC = 3     # pixel dtype of ctrl_vision_encoder_forward / the vision ops: uint8 [N][H][W][3]


CB_GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p)
CB_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)
CB_HALO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p)
CB_A2A = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p)


class ClipComm(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("all_gather", CB_GATHER), ("all_reduce_sum_f32", CB_REDUCE), ("halo_exchange", CB_HALO),
                ("user", C.c_void_p), ("ws_needed", C.c_int64), ("all_to_all", CB_A2A), ("next_lane", C.c_void_p)]


# every symbol include/ctrl_hip.h declares (tests check the library exports all of them)
ABI_VERSION = 11     # CTRL_ABI_VERSION of include/ctrl_hip.h
EXPORTS = [
    "ctrl_abi_version", "ctrl_last_error", "ctrl_prof_begin", "ctrl_prof_end", "ctrl_prof_count", "ctrl_prof_get",
    "ctrl_prof_launch_count", "ctrl_prof_launch_get",
    "ctrl_op_igemm", "ctrl_op_igemm_pinned", "ctrl_op_igemm_group", "ctrl_igemm_splitk_factor", "ctrl_igemm_splitk_ws_bytes", "ctrl_igemm_splitk_ticket_words", "ctrl_igemm_select", "ctrl_op_ffn", "ctrl_op_ffn_group", "ctrl_op_ffn_pack_w2", "ctrl_range_check", "ctrl_range_status", "ctrl_igemm_set_order", "ctrl_igemm_set_wide", "ctrl_group_launches", "ctrl_policy_set", "ctrl_policy_get", "ctrl_policy_count", "ctrl_policy_name", "ctrl_igemm_tile_of", "ctrl_op_flash_attn", "ctrl_op_flash_attn_group", "ctrl_attn_set_variant", "ctrl_attn_work_map", "ctrl_op_temporal_attn", "ctrl_op_gn_stats_floats", "ctrl_op_gn_stats", "ctrl_op_gn_apply", "ctrl_op_gn_apply_split", "ctrl_op_gn_fused_applies", "ctrl_op_gn_fused", "ctrl_op_pack_conv_w_dup", "ctrl_op_pack_conv_w_phase",
    "ctrl_op_gn_stats_group", "ctrl_op_gn_apply_group", "ctrl_op_gn_fused_group", "ctrl_gn_launch_shape", "ctrl_op_layernorm_group",
    "ctrl_op_layernorm_add", "ctrl_op_add_rowvec_clip", "ctrl_op_upsample2x_nhwc", "ctrl_op_fill_zero_group", "ctrl_op_linear_small_group",
    "ctrl_op_frameidx_sincos",
    "ctrl_op_layernorm", "ctrl_op_nchw_to_nhwc", "ctrl_op_nhwc_to_nchw", "ctrl_avgpool_nchw",
    "ctrl_op_timestep_sincos", "ctrl_op_linear_small", "ctrl_op_blend", "ctrl_op_add_rowvec",
    "ctrl_op_conv3x3_direct", "ctrl_op_conv3x3_direct_f32", "ctrl_op_conv3x3_rows_f32", "ctrl_op_conv3x3_small_mfma", "ctrl_op_pack_conv_w", "ctrl_op_pack_conv_w_direct", "ctrl_op_pack_linear_w",
    "ctrl_op_pack_vec",
    "ctrl_controlnet_param_count", "ctrl_controlnet_param_spec", "ctrl_controlnet_create",
    "ctrl_controlnet_destroy", "ctrl_controlnet_clone", "ctrl_controlnet_forward",
    "ctrl_adapter_param_count", "ctrl_adapter_param_spec", "ctrl_adapter_create", "ctrl_adapter_destroy",
    "ctrl_adapter_forward",
    "ctrl_adapter_forward_scatter", "ctrl_adapter_forward_clip_sharded", "ctrl_controlnet_text_cache", "ctrl_adapter_text_cache", "ctrl_controlnet_trim", "ctrl_adapter_trim", "ctrl_controlnet_selection", "ctrl_adapter_selection",
    "ctrl_step_forward", "ctrl_rccl_unique_id", "ctrl_rccl_comm_create", "ctrl_rccl_comm_destroy", "ctrl_rccl_comm_bind", "ctrl_rccl_comm_bytes_sent",
    "ctrl_router_weights", "ctrl_router_merge", "ctrl_prepare_images",
    "ctrl_text_encoder_create", "ctrl_text_encoder_destroy", "ctrl_text_encoder_forward", "ctrl_text_encoder_id_status",
    "ctrl_op_text_embed", "ctrl_op_text_attn", "ctrl_op_text_final_ln",
    "ctrl_text_encoder_create_ext", "ctrl_text_encoder_forward_ext", "ctrl_text_gemm_ws_bytes", "ctrl_op_text_gemm",
    "ctrl_op_text_gemm_finish", "ctrl_op_text_proj", "ctrl_op_text_store", "ctrl_op_vision_vt", "ctrl_op_text_final_ln_ext",
    "ctrl_vision_encoder_param_count", "ctrl_vision_encoder_param_spec", "ctrl_vision_encoder_create", "ctrl_vision_encoder_destroy",
    "ctrl_vision_encoder_forward", "ctrl_op_vision_patchify", "ctrl_op_vision_embed", "ctrl_op_vision_cls_ln", "ctrl_op_clip_resize_aa",
    "ctrl_vae_encoder_param_count", "ctrl_vae_encoder_param_spec", "ctrl_vae_encoder_create", "ctrl_vae_encoder_destroy",
    "ctrl_vae_encoder_forward", "ctrl_op_vae_row_softmax", "ctrl_op_vae_posterior",
    "ctrl_vae_decoder_param_count", "ctrl_vae_decoder_param_spec", "ctrl_vae_decoder_create", "ctrl_vae_decoder_destroy",
    "ctrl_vae_decoder_forward", "ctrl_vae_decoder_forward_strided", "ctrl_op_vae_dec_head", "ctrl_op_vae_dec_tail",
    "ctrl_vae_tdecoder_param_count", "ctrl_vae_tdecoder_param_spec", "ctrl_vae_tdecoder_create", "ctrl_vae_tdecoder_destroy",
    "ctrl_vae_tdecoder_forward", "ctrl_op_vae_time_conv",
    "ctrl_unet_st_param_count", "ctrl_unet_st_param_spec", "ctrl_unet_st_create", "ctrl_unet_st_destroy", "ctrl_unet_st_selection",
    "ctrl_unet_st_forward", "ctrl_op_unet_skip_join", "ctrl_op_unet_skip_join_split",
    "ctrl_unet2d_param_count", "ctrl_unet2d_param_spec", "ctrl_unet2d_create", "ctrl_unet2d_destroy", "ctrl_unet2d_selection",
    "ctrl_unet2d_set_text_cache", "ctrl_unet2d_forward", "ctrl_unet2d_workspace_bytes", "ctrl_op_unet_text_time",
    "ctrl_unet_i2v_param_count", "ctrl_unet_i2v_param_spec", "ctrl_unet_i2v_create", "ctrl_unet_i2v_destroy", "ctrl_unet_i2v_selection",
    "ctrl_unet_i2v_set_cond_cache", "ctrl_unet_i2v_forward", "ctrl_unet_i2v_workspace_bytes", "ctrl_op_i2v_latent_encoder",
    "ctrl_op_adaptive_avgpool_nhwc",
    "ctrl_sampler_create", "ctrl_sampler_destroy", "ctrl_sampler_reset", "ctrl_sampler_scalars", "ctrl_sampler_model_input",
    "ctrl_sampler_step", "ctrl_op_sampler_reset", "ctrl_op_sampler_model_input", "ctrl_op_sampler_step", "ctrl_op_sampler_launch_shape",
    "ctrl_op_merge_gather_group", "ctrl_op_merge_gather_launch_shape",
    "ctrl_op_pack_conv_w_ovf", "ctrl_op_pack_conv_w_dup_ovf", "ctrl_op_pack_conv_w_phase_ovf", "ctrl_op_pack_linear_w_ovf",
    "ctrl_op_nhwc_to_nchw_map", "ctrl_op_unet_conv_out", "ctrl_op_i2v_frames", "ctrl_op_vae_conv_in",
    "ctrl_op_canny_map", "ctrl_op_canny_hysteresis", "ctrl_op_canny_finish", "ctrl_canny", "ctrl_canny_ws_bytes", "ctrl_canny_launch_shape",
    "ctrl_hed_create", "ctrl_hed_destroy", "ctrl_hed_forward", "ctrl_hed_ws_bytes", "ctrl_op_hed_stem", "ctrl_op_hed_pool_proj",
    "ctrl_op_hed_fuse", "ctrl_op_hed_blur_f32", "ctrl_op_hed_nms", "ctrl_op_hed_blur_u8_bin",
    "ctrl_pidi_create", "ctrl_pidi_destroy", "ctrl_pidi_forward", "ctrl_pidi_ws_bytes", "ctrl_pidi_convert_pdc", "ctrl_pidi_launch_shape",
    "ctrl_op_pidi_stem", "ctrl_op_pidi_block", "ctrl_op_pidi_head_reduce", "ctrl_op_pidi_head_context", "ctrl_op_pidi_side",
    "ctrl_op_pidi_fuse",
    "ctrl_lineart_create", "ctrl_lineart_destroy", "ctrl_lineart_forward", "ctrl_lineart_ws_bytes", "ctrl_lineart_launch_shape",
    "ctrl_op_lineart_stem", "ctrl_op_in_stats_ws_floats", "ctrl_op_in_stats", "ctrl_op_in_apply", "ctrl_op_lineart_head",
    "ctrl_op_pack_convt_w_phase", "ctrl_op_pack_convt_w_phase_ovf",
]

_lib = None


def lib():
    """Loads libctrlhip.so once.  Raises if it is missing -- there is no CPU/eager fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libctrlhip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The HIP path has no fallback." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.ctrl_last_error.restype = C.c_char_p
        for name in EXPORTS:
            fn = getattr(_lib, name)
            if name not in ("ctrl_last_error", "ctrl_policy_get", "ctrl_policy_name", "ctrl_controlnet_destroy", "ctrl_adapter_destroy", "ctrl_rccl_comm_destroy", "ctrl_rccl_comm_bytes_sent",
                            "ctrl_text_encoder_destroy", "ctrl_vision_encoder_destroy", "ctrl_vae_encoder_destroy", "ctrl_vae_decoder_destroy",
                            "ctrl_vae_tdecoder_destroy", "ctrl_unet_st_destroy", "ctrl_unet2d_destroy", "ctrl_unet2d_workspace_bytes",
                            "ctrl_unet_i2v_destroy", "ctrl_unet_i2v_workspace_bytes", "ctrl_sampler_destroy", "ctrl_sampler_scalars",
                            "ctrl_canny_ws_bytes", "ctrl_hed_destroy", "ctrl_hed_ws_bytes", "ctrl_pidi_destroy", "ctrl_pidi_ws_bytes",
                            "ctrl_lineart_destroy", "ctrl_lineart_ws_bytes", "ctrl_op_in_stats_ws_floats"):
                fn.restype = C.c_int
        _lib.ctrl_policy_get.restype = C.c_char_p
        _lib.ctrl_policy_get.argtypes = [C.c_char_p]
        _lib.ctrl_policy_name.restype = C.c_char_p
        _lib.ctrl_policy_set.argtypes = [C.c_char_p, C.c_char_p]
        _lib.ctrl_controlnet_destroy.restype = None
        _lib.ctrl_adapter_destroy.restype = None
        _lib.ctrl_text_encoder_destroy.restype = None
        _lib.ctrl_op_text_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_text_attn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
        _lib.ctrl_op_text_final_ln.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_text_encoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_void_p]
        _lib.ctrl_text_encoder_forward_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_text_gemm_ws_bytes.restype = C.c_int64
        _lib.ctrl_text_gemm_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.ctrl_op_text_gemm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.ctrl_op_text_gemm_finish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_int, C.c_int64, C.c_void_p]
        _lib.ctrl_op_text_proj.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_op_text_store.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        _lib.ctrl_op_vision_vt.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_text_final_ln_ext.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                                   C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_vision_encoder_destroy.restype = None
        _lib.ctrl_vision_encoder_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_vision_encoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_vision_patchify.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p]
        _lib.ctrl_op_vision_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_vision_cls_ln.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_clip_resize_aa.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_vae_encoder_destroy.restype = None
        _lib.ctrl_vae_encoder_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_vae_encoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_row_softmax.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_posterior.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_vae_decoder_destroy.restype = None
        _lib.ctrl_vae_decoder_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_vae_decoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                                  C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_vae_decoder_forward_strided.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                                          C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_dec_head.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_dec_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_vae_tdecoder_destroy.restype = None
        _lib.ctrl_vae_tdecoder_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_vae_tdecoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                                   C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_time_conv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_int, C.c_void_p]
        _lib.ctrl_unet_st_destroy.restype = None
        _lib.ctrl_unet_st_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_unet_st_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_unet_skip_join.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        _lib.ctrl_op_unet_skip_join_split.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_unet2d_destroy.restype = None
        _lib.ctrl_unet2d_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_unet2d_set_text_cache.argtypes = [C.c_void_p, C.c_int]
        _lib.ctrl_unet2d_workspace_bytes.restype = C.c_int64
        _lib.ctrl_unet2d_workspace_bytes.argtypes = [C.c_void_p]
        _lib.ctrl_unet2d_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                             C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_unet_text_time.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                                C.c_void_p]
        _lib.ctrl_unet_i2v_destroy.restype = None
        _lib.ctrl_unet_i2v_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_unet_i2v_set_cond_cache.argtypes = [C.c_void_p, C.c_int]
        _lib.ctrl_unet_i2v_workspace_bytes.restype = C.c_int64
        _lib.ctrl_unet_i2v_workspace_bytes.argtypes = [C.c_void_p]
        _lib.ctrl_unet_i2v_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                               C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_i2v_latent_encoder.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_adaptive_avgpool_nhwc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_int, C.c_void_p]
        _lib.ctrl_sampler_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.ctrl_sampler_destroy.restype = None
        _lib.ctrl_sampler_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_sampler_reset.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ctrl_sampler_scalars.restype = C.c_void_p
        _lib.ctrl_sampler_scalars.argtypes = [C.c_void_p]
        _lib.ctrl_sampler_model_input.argtypes = [C.c_void_p, C.POINTER(SamplerDesc), C.c_int, C.c_void_p]
        _lib.ctrl_sampler_step.argtypes = [C.c_void_p, C.POINTER(SamplerDesc), C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_sampler_reset.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ctrl_op_sampler_model_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SamplerDesc), C.c_int, C.c_void_p]
        _lib.ctrl_op_sampler_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SamplerDesc), C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_sampler_launch_shape.argtypes = [C.POINTER(SamplerDesc), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int)]
        _mg = [C.POINTER(MergeSlot), C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_int,
               C.c_int, C.c_int]
        _lib.ctrl_op_merge_gather_group.argtypes = _mg + [C.c_void_p]
        _lib.ctrl_op_merge_gather_launch_shape.argtypes = _mg + [C.POINTER(C.c_int)] * 3
        _lib.ctrl_op_pack_conv_w_ovf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pack_conv_w_dup_ovf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pack_conv_w_phase_ovf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pack_linear_w_ovf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_nhwc_to_nchw_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_unet_conv_out.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_i2v_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_vae_conv_in.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_canny_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_canny_hysteresis.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int),
                                                  C.POINTER(C.c_int), C.c_void_p]
        _lib.ctrl_op_canny_finish.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_canny.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]
        _lib.ctrl_canny_ws_bytes.restype = C.c_int64
        _lib.ctrl_canny_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.ctrl_canny_launch_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.ctrl_hed_create.argtypes = [C.POINTER(HedConfig), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.ctrl_hed_destroy.restype = None
        _lib.ctrl_hed_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_hed_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p]
        _lib.ctrl_hed_ws_bytes.restype = C.c_int64
        _lib.ctrl_hed_ws_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        _lib.ctrl_op_hed_stem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_hed_pool_proj.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        _lib.ctrl_op_hed_fuse.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_hed_blur_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_hed_nms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_hed_blur_u8_bin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_pidi_create.argtypes = [C.POINTER(PidiConfig), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.ctrl_pidi_destroy.restype = None
        _lib.ctrl_pidi_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_pidi_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p]
        _lib.ctrl_pidi_ws_bytes.restype = C.c_int64
        _lib.ctrl_pidi_ws_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        _lib.ctrl_pidi_convert_pdc.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float)]
        _lib.ctrl_pidi_launch_shape.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.ctrl_op_pidi_stem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pidi_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pidi_head_reduce.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        _lib.ctrl_op_pidi_head_context.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        _lib.ctrl_op_pidi_side.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _lib.ctrl_op_pidi_fuse.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        _lib.ctrl_lineart_create.argtypes = [C.POINTER(LineartConfig), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.ctrl_lineart_destroy.restype = None
        _lib.ctrl_lineart_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_lineart_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p]
        _lib.ctrl_lineart_ws_bytes.restype = C.c_int64
        _lib.ctrl_lineart_ws_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        _lib.ctrl_lineart_launch_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.ctrl_op_lineart_stem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_in_stats_ws_floats.restype = C.c_int64
        _lib.ctrl_op_in_stats_ws_floats.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.ctrl_op_in_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_in_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ctrl_op_lineart_head.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        _lib.ctrl_op_pack_convt_w_phase.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_pack_convt_w_phase_ovf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ctrl_rccl_comm_destroy.restype = None
        _lib.ctrl_rccl_comm_destroy.argtypes = [C.c_void_p]
        _lib.ctrl_rccl_comm_bytes_sent.restype = C.c_int64
        _lib.ctrl_rccl_comm_bytes_sent.argtypes = [C.c_void_p]
        _lib.ctrl_rccl_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _lib.ctrl_rccl_comm_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        _lib.ctrl_rccl_unique_id.argtypes = [C.c_void_p]
        _lib.ctrl_op_gn_stats_floats.restype = C.c_size_t
        for nm in ("ctrl_op_gn_stats_group", "ctrl_op_gn_apply_group", "ctrl_op_gn_fused_group", "ctrl_op_layernorm_group",
                   "ctrl_op_linear_small_group"):
            getattr(_lib, nm).argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_gn_launch_shape.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.ctrl_op_layernorm_add.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p]
        _lib.ctrl_op_add_rowvec_clip.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_void_p]
        _lib.ctrl_op_add_rowvec.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p]
        _lib.ctrl_op_linear_small.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_upsample2x_nhwc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_op_fill_zero_group.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_op_frameidx_sincos.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ctrl_igemm_splitk_ws_bytes.restype = C.c_int64
        _lib.ctrl_igemm_splitk_ws_bytes.argtypes = [C.c_void_p, C.c_int]
        _lib.ctrl_igemm_splitk_ticket_words.restype = C.c_int64
        _lib.ctrl_igemm_splitk_ticket_words.argtypes = [C.c_void_p, C.c_int]
        _lib.ctrl_igemm_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        _lib.ctrl_op_ffn.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ctrl_op_ffn_group.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ctrl_op_conv3x3_direct_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p]
        _lib.ctrl_op_conv3x3_rows_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p]
        if _lib.ctrl_abi_version() != ABI_VERSION:
            raise RuntimeError("libctrlhip ABI version mismatch")
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().ctrl_last_error()
        raise RuntimeError("libctrlhip: " + (msg.decode() if msg else "unknown error"))


def range_check(on=None):
    """fp16 range check of the activations (debug aid for real checkpoints): range_check(True / False) switches it, range_check() queries.
    While on (also: CTRL_CHECK_FINITE=1), every forward of the module mirrors ends with range_status() and raises RuntimeError when a
    GEMM / convolution epilogue wrote an fp16 inf / nan (an activation beyond 65504)."""
    return bool(lib().ctrl_range_check(-1 if on is None else (1 if on else 0)))


def raise_if_out_of_range(what):
    """called by the module mirrors after a forward; synchronises only while the check is on, and never during a graph capture"""
    import torch
    if not lib().ctrl_range_check(-1) or torch.cuda.is_current_stream_capturing():
        return
    if lib().ctrl_range_status(1) == 1:
        raise RuntimeError("libctrlhip: %s produced a non-finite fp16 activation (a value beyond the fp16 range, |x| > 65504, or a NaN): "
                           "the fp16-operand path cannot represent this checkpoint's activations" % what)


def dtype_code(t):
    import torch
    if t == torch.float32:
        return F32
    if t == torch.float16:
        return F16
    if t == torch.bfloat16:
        return BF16
    raise ValueError("unsupported dtype %s (float32, float16, bfloat16 are supported)" % t)


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
