"""ctypes binding of libmmskin_hip.so (the C ABI declared in include/mmskin.h).

There is no CPU fallback: if the shared library is missing or a call fails, the
caller gets an exception.  PyTorch is used only for device memory, streams and
autograd plumbing around these calls.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libmmskin_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "mmskin.h")

F32, BF16 = 0, 1
LINEAR_SMALL, LINEAR_BIG_F32, LINEAR_BIG_BF16, LINEAR_PADDED_BF16 = 0, 1, 2, 3   # mmskin_linear_route (MMSKIN_LINEAR_* in mmskin.h)
WG_STAGED, WG_TAPS3, WG_RING, WG_RING3 = 0, 1, 2, 3   # mmskin_conv_wgrad_plan family (MMSKIN_WG_* in mmskin.h)
WGR_DIRECT, WGR_LANES = 0, 1                          # ... and reduce
CG_TILE128, CG_BIG256, CG_PIPE, CG_C64, CG_STEM7 = 0, 1, 2, 3, 4   # mmskin_conv_route family (MMSKIN_CG_* in mmskin.h)

_lib = None

c_f = ctypes.c_void_p          # device pointers travel as void*
_i, _i64, _f = ctypes.c_int, ctypes.c_int64, ctypes.c_float
_u64, _d = ctypes.c_uint64, ctypes.c_double
_P = ctypes.c_void_p

_SIGNATURES = {
    "mmskin_last_error": (ctypes.c_char_p, []),
    "mmskin_version": (_i, []),
    "mmskin_backbone_create": (_i, [ctypes.c_char_p, _i, _i, _i, _i, ctypes.POINTER(_P)]),
    "mmskin_backbone_destroy": (None, [_P]),
    "mmskin_backbone_num_tensors": (_i, [_P, _i]),
    "mmskin_backbone_tensor_info": (_i, [_P, _i, _i, ctypes.c_char_p, _i, ctypes.POINTER(_i64),
                                         ctypes.POINTER(_i64), ctypes.POINTER(_i), ctypes.POINTER(_i64)]),
    "mmskin_backbone_param_numel": (_i64, [_P]),
    "mmskin_backbone_buffer_numel": (_i64, [_P]),
    "mmskin_backbone_workspace_bytes": (_i64, [_P]),
    "mmskin_backbone_feature_dim": (_i, [_P]),
    "mmskin_backbone_feature_hw": (_i, [_P, _P, _P]),
    "mmskin_backbone_set_option": (_i, [_P, ctypes.c_char_p, _i]),
    "mmskin_backbone_set_pointer": (_i, [_P, ctypes.c_char_p, _P]),
    "mmskin_backbone_num_grad_segments": (_i, [_P, ctypes.POINTER(ctypes.c_int)]),
    "mmskin_backbone_grad_segment": (_i, [_P, _i, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "mmskin_backbone_wait_grad_segment": (_i, [_P, _i, _P]),
    "mmskin_backbone_last_conv_shape": (_i, [_P, _P, _P, _P]),
    "mmskin_backbone_last_conv_export": (_i, [_P, _P, _P, _P]),
    "mmskin_backbone_last_conv_grad": (_i, [_P, _P, _P, _P, _P]),
    "mmskin_mdnet_fuse_forward": (_i, [_P] * 5 + [_i64, _i, _P]),
    "mmskin_mdnet_fuse_backward": (_i, [_P] * 9 + [_i64, _i, _P]),
    "mmskin_backbone_profile_enable": (_i, [_P, _i]),
    "mmskin_backbone_profile_read": (_i, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64)]),
    "mmskin_backbone_num_units": (_i, [_P]),
    "mmskin_backbone_unit_info": (_i, [_P, _i, ctypes.c_char_p, _i, ctypes.POINTER(_i64)]),
    "mmskin_backbone_unit_flags": (_i, [_P, _i, ctypes.POINTER(_i)]),
    "mmskin_backbone_forward": (_i, [_P, _P, _P, _P, _P, _P, _i, _P]),
    "mmskin_backbone_forward_u8": (_i, [_P, _P, _P, _P, _P, _P, _P, _i, _P]),
    "mmskin_backbone_backward": (_i, [_P, _P, _P, _P, _P, _P]),
    "mmskin_conv2d_workspace_bytes": (_i64, [_i] * 9),
    "mmskin_conv2d_forward": (_i, [_P, _P, _P] + [_i] * 10 + [_P, _P]),
    "mmskin_conv2d_time": (ctypes.c_double, [_i] * 11 + [_P, _P]),
    "mmskin_conv2d_wgrad_time": (ctypes.c_double, [_i] * 11 + [_P, _P]),
    "mmskin_conv2d_dgrad_time": (ctypes.c_double, [_i] * 11 + [_P, _P]),
    "mmskin_conv2d_backward": (_i, [_P] * 5 + [_i] * 10 + [_P, _P]),
    "mmskin_conv_pipe_launches": (_i64, []),
    "mmskin_wgrad_ring_launches": (_i64, []),
    "mmskin_conv_wgrad_plan": (_i, [_i] * 10 + [_P]),
    "mmskin_conv_wgrad_slab_check": (_i, [_i] * 10 + [_i64]),
    "mmskin_conv_route": (_i, [_i] * 12 + [_P]),
    "mmskin_conv3x3_c64_launches": (_i64, []),
    "mmskin_stem7x7_launches": (_i64, []),
    "mmskin_conv2d_dgrad_fused_rows": (_i, [_i] * 9),
    "mmskin_conv2d_dgrad_fused": (_i, [_P] * 8 + [_i] * 9 + [_P, _P]),
    "mmskin_conv2d_dgrad_epilogue_workspace_bytes": (_i64, [_i] * 9),
    "mmskin_conv2d_dgrad_epilogue": (_i, [_P] * 13 + [_i] * 11 + [_P, _P]),
    "mmskin_conv2d_forward_epilogue_workspace_bytes": (_i64, [_i] * 9),
    "mmskin_conv2d_forward_epilogue_stat_rows": (_i, [_i] * 9),
    "mmskin_conv2d_forward_epilogue": (_i, [_P] * 10 + [_i] * 11 + [_P, _P]),
    "mmskin_wgrad3_ring_launches": (_i64, []),
    "mmskin_abn_workspace_bytes": (_i64, [_i] * 5),
    "mmskin_abn_backward": (_i, [_P] * 6 + [_i] * 5 + [_P, _P, _P, _P]),
    "mmskin_adam_step": (_i, [_P] * 4 + [_i64] + [ctypes.c_double] * 5 + [_i64, _P]),
    "mmskin_abn_backward_kept_gram": (_i, [_P] * 6 + [_i] * 5 + [_P, _P, _P, _P]),
    "mmskin_conv1x1_gram_stats": (_i, [_P, _P] + [_i] * 5 + [_P, _P, _P, _P]),
    "mmskin_batchnorm_workspace_bytes": (_i64, [_i] * 4),
    "mmskin_batchnorm_forward": (_i, [_P] * 8 + [_i] * 4 + [_f, _f, _i, _i, _P, _P]),
    "mmskin_batchnorm_backward": (_i, [_P] * 9 + [_i] * 6 + [_P, _P]),
    "mmskin_dwconv2d_workspace_bytes": (_i64, [_i] * 6),
    "mmskin_dwconv2d_forward": (_i, [_P] * 3 + [_i] * 8 + [_P, _P]),
    "mmskin_dwconv2d_backward": (_i, [_P] * 5 + [_i] * 8 + [_P, _P]),
    "mmskin_batchnorm_act_workspace_bytes": (_i64, [_i] * 4),
    "mmskin_batchnorm_act_forward": (_i, [_P] * 9 + [_i] * 4 + [_f, _f, _i, _i, _P, _P]),
    "mmskin_batchnorm_act_backward": (_i, [_P] * 11 + [_i] * 7 + [_P, _P]),
    "mmskin_bn_apply_rows": (_i, [_P] * 8 + [_i64, _i, _i, _f, _i, _P]),
    "mmskin_bn_bwd_apply_rows": (_i, [_P] * 5 + [_i] + [_P] * 5 + [_i64, _i, _i, _P]),
    "mmskin_se_workspace_bytes": (_i64, [_i] * 4),
    "mmskin_se_forward": (_i, [_P] * 6 + [_i] * 6 + [_P, _P]),
    "mmskin_se_backward": (_i, [_P] * 11 + [_i] * 6 + [_P, _P]),
    "mmskin_sd_workspace_bytes": (_i64, [_i, _i64]),
    "mmskin_sd_forward": (_i, [_P] * 4 + [_i, _i64, _i, _P, _P]),
    "mmskin_sd_backward": (_i, [_P] * 3 + [_i, _i64, _i, _P, _P]),
    "mmskin_dense_block_workspace_bytes": (_i64, [_i] * 5),
    "mmskin_dense_block_param_numel": (_i64, [_i] * 2),
    "mmskin_dense_block_forward": (_i, [_P] * 5 + [_i] * 7 + [_P, _P]),
    "mmskin_dense_block_backward": (_i, [_P] * 5 + [_i] * 6 + [_P, _P]),
    "mmskin_dense_transition_workspace_bytes": (_i64, [_i] * 5),
    "mmskin_dense_transition_forward": (_i, [_P] * 6 + [_i] * 7 + [_P, _P]),
    "mmskin_dense_transition_backward": (_i, [_P] * 7 + [_i] * 6 + [_P, _P]),
    "mmskin_slice_stats_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "mmskin_col_reduce_scratch_doubles": (_i64, [_i64]),
    "mmskin_col_reduce_scratch_check": (_i, [_i, _i, _i, _i64]),
    "mmskin_slice_stats": (_i, [_P, _i64, _i, _i, _i, _P, _P, _i, _P, _P]),
    "mmskin_maxpool2_relu_workspace_bytes": (_i64, [_i] * 4),
    "mmskin_maxpool2_relu_forward": (_i, [_P] * 3 + [_i] * 5 + [_P, _P]),
    "mmskin_maxpool2_relu_backward": (_i, [_P] * 3 + [_i] * 5 + [_P, _P]),
    "mmskin_groupnorm8_relu_workspace_bytes": (_i64, [_i] * 6),
    "mmskin_groupnorm8_relu_forward": (_i, [_P] * 7 + [_i] * 6 + [_f, _i, _P, _P]),
    "mmskin_groupnorm8_relu_backward": (_i, [_P] * 7 + [_i] * 6 + [_f, _i, _P, _P]),
    "mmskin_groupnorm8_relu_gap_workspace_bytes": (_i64, [_i] * 6),
    "mmskin_groupnorm8_relu_gap_forward": (_i, [_P] * 6 + [_i] * 6 + [_f, _i, _P, _P]),
    "mmskin_groupnorm8_relu_gap_backward": (_i, [_P] * 7 + [_i] * 6 + [_f, _i, _P, _P]),
    "mmskin_adaptive_avgpool_workspace_bytes": (_i64, [_i] * 4),
    "mmskin_adaptive_avgpool_forward": (_i, [_P] * 2 + [_i] * 5 + [_P, _P]),
    "mmskin_adaptive_avgpool_backward": (_i, [_P] * 2 + [_i] * 5 + [_P, _P]),
    "mmskin_stem_workspace_bytes": (_i64, [_i] * 3),
    "mmskin_stem_forward": (_i, [_P] * 5 + [_i] * 3 + [_f, _i, _P, _P]),
    "mmskin_stem_backward": (_i, [_P] * 8 + [_i] * 3 + [_f, _i, _P, _P]),
    "mmskin_linear_forward": (_i, [_P] * 4 + [_i] * 4 + [_P]),
    "mmskin_linear_backward": (_i, [_P] * 8 + [_i] * 3 + [_P]),
    "mmskin_linear_gelu_backward": (_i, [_P] * 8 + [_i] * 3 + [_P]),
    "mmskin_linear_x16_pitch": (_i, [_i, _i, _i]),
    "mmskin_linear_route": (_i, [_i, _i, _i]),
    "mmskin_linear_forward_keep": (_i, [_P] * 6 + [_i] * 4 + [_P]),
    "mmskin_linear_backward_keep": (_i, [_P] * 9 + [_i] * 3 + [_P]),
    "mmskin_gelu_forward_bf16": (_i, [_P, _P, _i64, _i, _i, _P]),
    "mmskin_linear_forward_x16": (_i, [_P] * 5 + [_i] * 4 + [_P]),
    "mmskin_layernorm_forward": (_i, [_P] * 6 + [_i, _i, _f, _i, _P]),
    "mmskin_layernorm_backward": (_i, [_P] * 9 + [_i, _i, _i, _P]),
    "mmskin_sigmoid_gate_forward": (_i, [_P] * 3 + [_i64, _P]),
    "mmskin_sigmoid_gate_backward": (_i, [_P] * 5 + [_i64, _P]),
    "mmskin_gated_mix_forward": (_i, [_P] * 4 + [_i64, _P]),
    "mmskin_gated_mix_backward": (_i, [_P] * 7 + [_i64, _P]),
    "mmskin_metablock_gate_forward": (_i, [_P] * 4 + [_i64, _P]),
    "mmskin_metablock_gate_backward": (_i, [_P] * 7 + [_i64, _P]),
    "mmskin_dropout_forward": (_i, [_P] * 3 + [_i64, _f, _u64, _u64, _P]),
    "mmskin_attn_dropout_forward": (_i, [_P] * 3 + [_i64, _i, _f, _u64, _u64, _P]),
    "mmskin_dropout_backward": (_i, [_P] * 3 + [_i64, _f, _P]),
    "mmskin_concat2_forward": (_i, [_P] * 3 + [_i] * 3 + [_P]),
    "mmskin_concat2_backward": (_i, [_P] * 3 + [_i] * 3 + [_P]),
    "mmskin_attention_forward": (_i, [_P] * 5 + [_i] * 4 + [_f, _u64, _u64, _P]),
    "mmskin_attention_backward": (_i, [_P] * 8 + [_i] * 4 + [_f, _u64, _u64, _P]),
    "mmskin_bmm": (_i, [_P] * 3 + [_i] * 4 + [_i64] * 8 + [_P]),
    "mmskin_softmax_forward": (_i, [_P] * 4 + [_i64, _i, _i64, _f, _i, _P]),
    "mmskin_gelu_tanh_forward": (_i, [_P, _P, _i64, _P]),
    "mmskin_gelu_tanh_backward": (_i, [_P, _P, _P, _i64, _P]),
    "mmskin_colsum": (_i, [_P, _P, _i, _i, _P]),
    "mmskin_dwconv3_scratch_floats": (_i64, [_i, _i, _i, _i]),
    "mmskin_dwconv3_forward": (_i, [_P] * 4 + [_i] * 4 + [_P]),
    "mmskin_dwconv3_backward": (_i, [_P] * 7 + [_i] * 4 + [_P]),
    "mmskin_conv_pos_enc_forward": (_i, [_P] * 5 + [_i] * 4 + [_P]),
    "mmskin_conv_pos_enc_backward": (_i, [_P] * 8 + [_i] * 4 + [_P]),
    "mmskin_factor_attention_scratch_floats": (_i64, [_i] * 5),
    "mmskin_factor_attention_forward": (_i, [_P] * 11 + [_i] * 4 + [_P]),
    "mmskin_factor_attention_backward": (_i, [_P] * 18 + [_i] * 4 + [_P]),
    "mmskin_conv_pos_enc_tokens_scratch_floats": (_i64, [_i] * 4),
    "mmskin_conv_pos_enc_tokens_forward": (_i, [_P] * 4 + [_i] * 4 + [_P]),
    "mmskin_conv_pos_enc_tokens_backward": (_i, [_P] * 7 + [_i] * 4 + [_P]),
    "mmskin_scale_add_forward": (_i, [_P] * 4 + [_i64, _i, _P]),
    "mmskin_scale_mul": (_i, [_P] * 3 + [_i64, _i, _i, _P]),
    "mmskin_token_mean_forward": (_i, [_P, _P, _i, _i, _i, _i, _P]),
    "mmskin_token_mean_backward": (_i, [_P, _P, _i, _i, _i, _i, _P]),
    "mmskin_softmax_backward": (_i, [_P] * 3 + [_i64, _i, _f, _P]),
    "mmskin_add": (_i, [_P, _P, _P, _i64, _i64, _P]),
    "mmskin_gelu_forward": (_i, [_P, _P, _i64, _P]),
    "mmskin_gelu_backward": (_i, [_P, _P, _P, _i64, _P]),
    "mmskin_embedding_forward": (_i, [_P] * 3 + [_i] * 4 + [_P]),
    "mmskin_embedding_backward": (_i, [_P] * 3 + [_i] * 4 + [_P]),
    "mmskin_direct_conv2d_forward": (_i, [_P] * 4 + [_i] * 10 + [_P]),
    "mmskin_direct_conv2d_backward": (_i, [_P] * 5 + [_i] * 9 + [_P]),
    "mmskin_linear_forward_ex": (_i, [_P, _i, _P, _P, _P, _i, _i, _i, _i, _i, _P]),
    "mmskin_attention_rows_forward": (_i, [_P] * 5 + [_i] * 4 + [_P, _P, _f, _f, _u64, _u64, _P]),
    "mmskin_attention_rows_backward": (_i, [_P] * 9 + [_i] * 4 + [_P, _P, _f, _f, _u64, _u64, _P]),
    "mmskin_window_attention_forward": (_i, [_P] * 5 + [_i] * 6 + [_i64] * 4 + [_f, _f, _u64, _u64, _P]),
    "mmskin_window_attention_backward": (_i, [_P] * 9 + [_i] * 6 + [_i64] * 4 + [_f, _f, _u64, _u64, _P]),
    "mmskin_swin_attention_workspace_bytes": (_i64, [_i] * 5),
    "mmskin_swin_attention_forward": (_i, [_P] * 6 + [_i] * 8 + [_i64] * 4 + [_f, _f, _u64, _u64, _P]),
    "mmskin_swin_attention_backward": (_i, [_P] * 12 + [_i] * 8 + [_i64] * 4 + [_f, _f, _u64, _u64, _P]),
    "mmskin_channel_attention_scratch_floats": (_i64, [_i, _i, _i]),
    "mmskin_channel_attention_forward": (_i, [_P] * 6 + [_i] * 4 + [_i64] * 4 + [_f, _P]),
    "mmskin_channel_attention_backward": (_i, [_P] * 9 + [_i] * 4 + [_i64] * 4 + [_f, _P]),
    "mmskin_linear_lane": (_i, [_P, _i, _P, _i, _P, _P, _P, _f, _u64, _u64, _P, _i, _i, _i, _i, _i, _P]),
    "mmskin_layernorm_forward_mixed": (_i, [_P] * 5 + [_i, _i, _f, _P]),
    "mmskin_flash_attention_forward": (_i, [_P] * 7 + [_i] * 4 + [_P, _i, _f, _i, _f, _u64, _u64, _P]),
    "mmskin_flash_attention_backward": (_i, [_P] * 14 + [_i] * 4 + [_P, _f, _i, _f, _u64, _u64, _P]),
    "mmskin_set_linear_dtype": (_i, [_i]),
    "mmskin_get_linear_dtype": (_i, []),
    "mmskin_im2col_forward": (_i, [_P] + [_i] * 8 + [_P, _P]),
    "mmskin_im2col_backward": (_i, [_P] + [_i] * 8 + [_P, _P]),
    "mmskin_resize_u8": (_i, [_P, _i, _i, _i, _P, _i, _i, _P]),
    "mmskin_metadata_encode": (_i, [_P, _i, _P, _i, _P, _i, _P, _P, _f, _P, _i, _P]),
    "mmskin_train_augment_u8": (_i, [_P, _i, _i, _i, _P, _P, _P, _P]),
    "mmskin_scorecam_minmax": (_i, [_P] + [_i] * 5 + [_P, _P]),
    "mmskin_scorecam_mask": (_i, [_P] * 3 + [_i] * 8 + [_P, _P]),
    "mmskin_scorecam_combine": (_i, [_P] * 3 + [_i] * 6 + [_P, _P]),
    "mmskin_gradcam_weights": (_i, [_P] * 4 + [_i] * 6 + [_P, _P]),
    "mmskin_gradcam_map": (_i, [_P] * 3 + [_i] * 7 + [_P] * 3),
    "mmskin_faith_max_pixels": (_i, []),
    "mmskin_faith_rank": (_i, [_P, _i, _i, _P, _P]),
    "mmskin_faith_blur": (_i, [_P, _i, _i, _i, _P, _i, _P, _P]),
    "mmskin_faith_mean": (_i, [_P, _i, _i, _P, _P]),
    "mmskin_faith_perturb": (_i, [_P] * 5 + [_i] * 6 + [_P, _P]),
    "mmskin_faith_curves": (_i, [_P, _P, _i, _i, _i] + [_P] * 5),
    "mmskin_rise_masks": (_i, [_u64, _i, _i, _i, _d, _i, _i, _P, _P]),
    "mmskin_rise_apply": (_i, [_P, _P, _i, _i, _i, _u64, _i, _d, _i, _i64, _i, _i, _P, _P]),
    "mmskin_rise_workspace_bytes": (_i64, [_i, _i]),
    "mmskin_rise_accumulate": (_i, [_P, _P, _P] + [_i] * 4 + [_u64, _i, _d, _i] + [_P] * 6),
    "mmskin_metadata_variants": (_i, [_P, _i, _P, _P, _i, _P, _i, _P, _P, _f, _P, _P, _i, _P, _P, _P, _i, _i, _P]),
    "mmskin_sweep_reduce": (_i, [_P, _i, _P, _P, _i, _i, _i] + [_P] * 7 + [_P]),
    "mmskin_shapley_rows": (_i64, [_i] * 4),
    "mmskin_shapley_coalitions": (_i, [_P, _P, _i, _P, _P, _i, _i, _P, _P, _i, _i, _P, _P, _f, _P, _P, _i, _i64, _i64, _P, _i, _P]),
    "mmskin_shapley_reduce": (_i, [_P, _i, _i] + [_i] * 5 + [_i64, _i64, _P, _i] + [_P] * 6 + [_P]),
    "mmskin_lime_accumulator_doubles": (_i64, [_i] * 4),
    "mmskin_lime_solve_workspace_bytes": (_i64, [_i] * 3),
    "mmskin_lime_neighbourhood": (_i, [_P, _i, _i, _P, _P, _i, _i, _u64, _i64, _i, _i64, _i64, _P, _i, _P, _i, _P]),
    "mmskin_lime_reduce": (_i, [_P, _i, _P, _i, _P, _i, _i, _P, _P] + [_i] * 4 + [_i64, _i64, _P, _P]),
    "mmskin_lime_solve": (_i, [_P, _P, _i, _P, _P] + [_i] * 5 + [_P] * 9),
    "mmskin_permutation_indices": (_i, [_u64, _i, _i, _i, _P, _P]),
    "mmskin_permuted_rows": (_i, [_P, _i, _P, _P, _i, _i, _i, _i, _i64, _i64, _P, _P]),
    "mmskin_permutation_scores": (_i, [_P, _P, _i, _i, _i, _i, _i64, _i64, _P, _P, _P]),
    "mmskin_permutation_finalize": (_i, [_P, _P, _P, _i, _i, _i, _P, _P, _P, _P, _P]),
    "mmskin_bootstrap_metric_columns": (_i, [_i]),
    "mmskin_bootstrap_weights": (_i, [_u64, _i, _i, _i, _i, _P, _P, _P, _i, _i, _P, _P]),
    "mmskin_bootstrap_replicates": (_i, [_u64, _i, _i, _i, _i] + [_P] * 7 + [_i, _i, _P, _P, _P]),
    "mmskin_bootstrap_finalize": (_i, [_P, _P, _i, _i, _d, _d, _P, _P, _P]),
    "mmskin_bootstrap_compare": (_i, [_P, _P, _i, _i, _d, _d, _P, _P, _P, _P]),
    "mmskin_subgroup_metric_columns": (_i, [_i]),
    "mmskin_subgroup_replicates": (_i, [_u64, _i, _i, _i, _i, _i] + [_P] * 9 + [_i, _i, _P, _P, _P]),
    "mmskin_subgroup_finalize": (_i, [_P, _P, _i, _i, _i, _i64, _d, _d, _P, _P, _P]),
    "mmskin_subgroup_gaps": (_i, [_P, _i, _i, _i, _d, _d] + [_P] * 6),
    "mmskin_calibration_metric_columns": (_i, [_i]),
    "mmskin_calibration_sums_scratch_doubles": (_i64, [_i, _i]),
    "mmskin_temperature_scratch_doubles": (_i64, [_i, _i]),
    "mmskin_calibration_codes": (_i, [_P, _P, _i, _i, _P, _i, _P, _P, _P, _P]),
    "mmskin_calibration_bins": (_i, [_i, _i, _i, _P, _P, _P, _P, _i, _P, _P]),
    "mmskin_calibration_sums": (_i, [_P, _P, _i, _i, _P, _i, _P, _P, _P]),
    "mmskin_calibration_finalize": (_i, [_P, _P, _i, _i, _i, _d, _d, _P, _P, _P]),
    "mmskin_temperature_stats": (_i, [_P, _i, _P, _i, _i, ctypes.POINTER(_d), _i, _P, _P, _P]),
    "mmskin_temperature_apply": (_i, [_P, _i, _i, _i, _d, _P, _P]),
    "mmskin_criterion_scratch_floats": (_i64, [_i, _i, _i]),
    "mmskin_criterion_forward": (_i, [_P, _i, _P, _P, _i, _i, _f, _i, _i] + [_P] * 6),
    "mmskin_criterion_backward": (_i, [_P, _i, _P, _P, _i, _i, _f, _i, _i] + [_P] * 4),
    "mmskin_ovr_auc_counts": (_i, [_P, _P, _i64, _i, _P, _P]),
    "mmskin_ovr_curves_scratch_ints": (_i64, [_i64, _i]),
    "mmskin_ovr_curves_summary_columns": (_i, [_i, _i]),
    "mmskin_ovr_curves": (_i, [_P, _P, _i64, _i] + [_P] * 7),
    "mmskin_ovr_curves_summary": (_i, [_P] * 5 + [_i64, _i, _P, _i, _P, _i, _P, _P]),
    "mmskin_dihedral_views": (_i, [_P, _P] + [_i] * 6 + [_P]),
    "mmskin_uncertainty_reduce": (_i, [_P, _i64, _i64, _i, _i, _i] + [_P] * 5 + [_P]),
    "mmskin_risk_coverage": (_i, [_P, _P, _i, _P, _P]),
    "mmskin_risk_coverage_summary": (_i, [_P, _P, _i, _P, _P]),
    "mmskin_conformal_count_columns": (_i, [_i]),
    "mmskin_conformal_metric_columns": (_i, [_i]),
    "mmskin_conformal_workspace_bytes": (_i64, [_i, _i, _i]),
    "mmskin_conformal_score": (_i, [_P, _i, _i64, _i, _i, _i, _d, _i, _u64, _i64, _P, _P, _P, _P]),
    "mmskin_conformal_apply": (_i, [_P, _i, _i64, _i, _i, _i, _d, _i, _u64, _i64, _P, _P, _P, _P]),
    "mmskin_conformal_study": (_i, [_u64, _i, _i, _i, _i, _d, _i] + [_P] * 5 + [_i, _i, _P, _P, _P, _P]),
    "mmskin_conformal_fit": (_i, [_i, _i, _d, _i] + [_P] * 6),
    "mmskin_conformal_finalize": (_i, [_P, _P, _i, _i, _i, _d, _d, _P, _P, _P]),
    "mmskin_pool_gap_forward":(_i, [_P] * 3 + [_i] * 5 + [_P]),
    "mmskin_pool_gap_backward": (_i, [_P] * 3 + [_i] * 5 + [_P]),
    "mmskin_star_relu_forward_bf16": (_i, [_P] * 4 + [_i64, _i, _i, _P]),
    "mmskin_linear_star_relu_backward_keep": (_i, [_P] * 9 + [_i] * 3 + [_P]),
    "mmskin_star_relu_forward": (_i, [_P] * 4 + [_i64, _P]),
    "mmskin_star_relu_backward": (_i, [_P] * 5 + [_i64, _P]),
    "mmskin_dw7_star_scratch_floats": (_i64, [_i] * 4),
    "mmskin_dw7_star_forward": (_i, [_P] * 5 + [_i] * 4 + [_P]),
    "mmskin_dw7_star_backward": (_i, [_P] * 9 + [_i] * 4 + [_P]),
}


class MMSkinError(RuntimeError):
    pass


def declared_symbols():
    """Every function name include/mmskin.h declares (used by the export test)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(mmskin_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load the shared library (once) and attach prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MMSkinError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (or `make -C "
            f"{os.path.join(os.path.dirname(_HERE), 'csrc')}`).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().mmskin_last_error()
        raise MMSkinError(f"mmskin error {rc}: {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = None


def stream():
    """hipStream_t of torch's current stream on the current device (raw handle: torch.cuda.current_stream() builds a Stream object
    and resolves the device index in Python, ~8 us per op on a launch-bound step)"""
    global _raw_stream
    if _raw_stream is None:
        import torch
        get, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        if get is not None and dev is not None:
            _raw_stream = lambda: get(dev())
        else:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
    return ctypes.c_void_p(_raw_stream())


_fns = {}


def call(name, *args):
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    rc = fn(*args)
    if rc != 0:
        check(rc)
