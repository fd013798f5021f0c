"""ctypes binding of ``libsis_hip.so`` (C ABI declared in ``include/sis_hip.h``).

This is the only place where Python touches the native library.  There is NO fallback: when the
shared object is missing, or a tensor is not on a HIP device, the wrappers raise ``RuntimeError``
(the reference's ops raise ``RuntimeError("... must be a CUDA tensor")`` in the same situations,
networks/stylegan2/op/fused_bias_act.cpp:13-14, upfirdn2d.cpp:15-16).

PyTorch is used for device memory and streams only: every wrapper takes ``torch.Tensor``s,
passes ``data_ptr()`` and the current HIP stream, and returns freshly allocated tensors, mirroring
the ownership rules of the reference extension (outputs owned by the caller, inputs borrowed and
made contiguous, kernels enqueued on the current stream, no host sync).
"""
import collections
import ctypes
import os
import weakref

import torch

from . import backward_scope

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", os.environ.get("SIS_HIP_LIB", "libsis_hip.so"))  # (override: same-box A/B
# timing of another build of the same library, tools/build_variant.sh)

_lib = None

F32, F64, F16, BF16 = 0, 1, 2, 3
_DTYPE_CODE = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16}

_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_d = ctypes.c_double

_SIGNATURES = {
    "sis_version": ([], _i),
    "sis_last_error": ([], ctypes.c_char_p),
    "sis_fused_bias_act": ([_vp, _vp, _vp, _vp, _i, _i64, _i64, _i64, _i, _i, _f, _f, _vp], _i),
    "sis_upfirdn2d_out_size": ([_i] * 6, _i),
    "sis_upfirdn2d": ([_vp, _vp, _vp] + [_i] * 15 + [_vp], _i),
    "sis_pixel_norm": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_equal_linear": ([_vp, _vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp], _i),
    "sis_truncate": ([_vp, _vp, _vp, _f, _i, _i, _vp], _i),
    "sis_modulation_batch": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp], _i),
    "sis_demod_batch": ([_vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "sis_modconv_prepack": ([_vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "sis_modconv_demod": ([_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp], _i),
    "sis_modconv2d": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp] + [_i] * 7 + [_vp, _vp, _i64, _vp], _i),
    "sis_head_gemm_tile": ([], _i),
    "sis_modconv_prepack_wino": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_modconv_prepack_wino24": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_modconv_wino24_eligible": ([_i] * 4, _i),
    "sis_modconv2d_wino24": ([_vp] * 6 + [_i64, _vp, _vp] + [_i] * 7 + [_vp], _i),
    "sis_modconv2d_wino24_rgb": ([_vp] * 7 + [_i64, _vp, _vp, _vp, _vp, _f] + [_i] * 7 + [_vp], _i),
    "sis_modconv_prepack_wino44": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_modconv_wino44_eligible": ([_i] * 4, _i),
    "sis_modconv2d_wino44": ([_vp] * 6 + [_i64, _vp, _vp] + [_i] * 7 + [_vp], _i),
    "sis_modconv2d_wino44_rgb": ([_vp] * 7 + [_i64, _vp, _vp, _vp, _vp, _f] + [_i] * 7 + [_vp], _i),
    "sis_rgb_finish": ([_vp] * 5 + [_i] * 9 + [_vp], _i),
    "sis_modconv_bf16_eligible": ([_i] * 4, _i),
    "sis_modconv_bf16_packed_elems": ([_i] * 2, _i64),
    "sis_modconv_prepack_bf16": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_modconv2d_bf16": ([_vp] * 6 + [_i64, _vp, _vp] + [_i] * 6 + [_vp], _i),
    "sis_last_kernel": ([], ctypes.c_char_p),
    "sis_conv3x3_prepack": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "sis_conv3x3_prepack_both": ([_vp, _vp, _vp, _i, _i, _vp], _i),
    "sis_conv3x3_prepack_multi": ([_vp, _i, _i, _vp], _i),
    "sis_conv3x3_eligible": ([_i] * 5, _i),
    "sis_upsample_bilinear": ([_vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _vp], _i),
    "sis_upsample_bilinear_strided": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i64, _i, _vp], _i),
    "sis_gemm_bf16_workspace_bytes": ([_i, _i, _i], _i64),
    "sis_gemm_bf16": ([_vp] * 4 + [_i] * 8 + [_vp] * 3 + [_i] + [_vp] * 3 + [_i, _f, _i, _vp, _i64, _i, _vp], _i),
    "sis_gemm_bf16_wgrad_bias": ([_vp] * 4 + [_i] * 6 + [_vp, _i64, _i, _vp], _i),
    "sis_gemm_bf16_wgrad_multi_workspace_bytes": ([_i, _i, _i], _i64),
    "sis_gemm_bf16_wgrad_bias_multi": ([_vp] * 4 + [_i] * 6 + [_vp, _i64, _i, _vp], _i),
    "sis_gemm_bf16_batched": ([_vp] * 3 + [_i] * 9 + [_i64] * 3 + [_i, _vp, _i64, _i, _vp], _i),
    "sis_layer_norm_bwd_fused": ([_vp] * 9 + [_i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _vp], _i),
    "sis_attention_fwd": ([_vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "sis_attention_bwd": ([_vp] * 6 + [_i, _i, _i, _vp], _i),
    "sis_ce_dice_workspace_floats": ([_i], _i),
    "sis_ce_dice_fwd": ([_vp] * 4 + [_i, _vp, _i, _i, _i, _vp], _i),
    "sis_ce_dice_bwd": ([_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "sis_dropout_advance": ([_vp, _vp], _i),
    "sis_dropout_bwd_cast": ([_vp, _vp, _i64, _vp, _i, _f, _vp], _i),
    "sis_layer_norm_workspace_floats": ([_i], _i),
    "sis_layer_norm_bwd_fused_partial": ([_vp] * 7 + [_i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _vp], _i),
    "sis_layer_norm_bwd_parts": ([_i], _i),
    "sis_layer_norm_param_reduce_multi": ([_vp] * 5 + [_i, _vp], _i),
    "sis_column_sum_workspace_floats": ([_i], _i64),
    "sis_column_sum": ([_vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "sis_layer_norm_fwd": ([_vp] * 6 + [_i, _i, _i, _i, _f, _vp], _i),
    "sis_layer_norm_bwd": ([_vp] * 9 + [_i, _i, _i, _i, _vp], _i),
    "sis_weight_std_fwd": ([_vp, _vp, _vp, _i, _i, _i, _f, _vp], _i),
    "sis_group_norm_fwd": ([_vp] * 9 + [_i, _i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp], _i),
    "sis_group_norm_gate_bytes": ([_i, _i, _i], _i64),
    "sis_group_norm_workspace_floats": ([_i, _i, _i], _i64),
    "sis_batch_norm_fwd": ([_vp] * 9 + [_i] * 5 + [_f, _f, _i, _vp, _vp], _i),
    "sis_batch_norm_bwd": ([_vp] * 10 + [_i] * 6 + [_vp, _vp], _i),
    "sis_group_norm_bwd": ([_vp] * 13 + [_i] * 7 + [_vp, _vp, _vp], _i),
    "sis_weight_std_bwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp], _i),
    "sis_conv3x3_wgrad_eligible": ([_i] * 5 + [_i64], _i),
    "sis_conv3x3_wgrad": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_conv3x3_wgrad_multi": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_conv3x3": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_modconv2d_up": ([_vp] * 5 + [_i] * 6 + [_vp, _i64, _vp], _i),
    "sis_modconv_up_fir_supported": ([_i] * 6, _i),
    "sis_modconv_up_fir_prepack": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_modconv2d_up_fir": ([_vp] * 5 + [_i] * 6 + [_vp], _i),
    "sis_blur_noise_act": ([_vp, _vp, _vp, _vp, _i64, _vp, _vp] + [_i] * 10 + [_vp], _i),
    "sis_to_rgb": ([_vp] * 7 + [_i] * 9 + [_f, _vp], _i),
    "sis_conv1x1_wgrad_f32_supported": ([_i] * 4, _i),
    "sis_conv1x1_wgrad_f32_workspace": ([_i] * 4, _i64),
    "sis_conv1x1_wgrad_f32": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_conv1x1_wgrad_f32_multi": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_max_pool2d": ([_vp, _vp, _vp, _i, _i64] + [_i] * 8 + [_vp], _i),
    "sis_upsample_ce_workspace": ([_i] * 3, _i),
    "sis_upsample_ce_fwd": ([_vp] * 4 + [_i] * 6 + [_i64, _vp], _i),
    "sis_upsample_ce_bwd": ([_vp] * 4 + [_i] * 6 + [_i64, _vp], _i),
    "sis_sgd_chunk_elems": ([], _i),
    "sis_sgd_momentum": ([_vp, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _f, _i, _vp], _i),
    "sis_sgd_momentum_dev": ([_vp, _i, _vp, _vp], _i),
    "sis_ema_update": ([_vp, _vp, _f, _f, _i, _i, _vp], _i),
    "sis_transpose_bf16_multi": ([_vp, _i, _i, _vp], _i),
    "sis_transpose_batched": ([_vp, _vp, _i, _i, _i, _i, _vp], _i),
    "sis_half_dilation_taps": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_half_dilation_taps_bwd": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_emau_supported": ([_i] * 4, _i),
    "sis_emau_workspace_floats": ([_i] * 4, _i64),
    "sis_emau_forward": ([_vp] * 5 + [_i] * 5 + [_vp], _i),
    "sis_bn_workspace_floats": ([_i, _i, _i], _i64),
    "sis_bn_stats": ([_vp] * 6 + [_i, _i, _i, _f, _f, _vp], _i),
    "sis_bn_mask_words": ([_i, _i, _i], _i64),
    "sis_bn_act_fwd": ([_vp] * 7 + [_i, _i, _i, _i, _vp, _vp], _i),
    "sis_bn_fused_supported": ([_i] * 3, _i),
    "sis_bn_fused_fwd": ([_vp] * 9 + [_i, _i, _i, _f, _f, _i, _vp, _vp], _i),
    "sis_bn_act_bwd": ([_vp] * 11 + [_i, _i, _i, _i, _vp, _vp], _i),
    "sis_kmeans_assign": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "sis_kmeans_workspace_ints": ([_i, _i], _i64),
    "sis_kmeans_assign_ws": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_make_image_u8": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "sis_crop_patches_u8": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "sis_assemble_max": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "sis_conv_bf16_supported": ([_i] * 6, _i),
    "sis_conv_bf16_packed_elems": ([_i] * 7, _i64),
    "sis_conv_bf16_pack": ([_vp, _vp, _i] + [_i] * 7 + [_vp], _i),
    "sis_conv_bf16": ([_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp], _i),
    "sis_conv1x1_f32_supported": ([_i] * 3, _i),
    "sis_conv1x1_f32": ([_vp, _vp, _vp, _vp] + [_i] * 5 + [_vp], _i),
    "sis_conv1x1_f32_dgrad_add": ([_vp, _vp, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_conv_bf16_pack_both": ([_vp, _vp, _vp, _i] + [_i] * 5 + [_vp], _i),
    "sis_conv_bf16_wgrad_supported": ([_i] * 5 + [_i64], _i),
    "sis_conv_bf16_wgrad": ([_vp, _i, _vp, _vp] + [_i] * 5 + [_vp, _i64, _vp], _i),
    "sis_conv_bf16_wgrad_multi": ([_vp, _i, _vp, _vp] + [_i] * 6 + [_vp, _i64, _vp], _i),
    "sis_stem_conv_supported": ([_i] * 7, _i),
    "sis_stem_conv_packed_elems": ([], _i64),
    "sis_stem_conv_pack": ([_vp, _vp, _i, _vp], _i),
    "sis_stem_conv_fwd": ([_vp, _vp, _i, _vp, _i, _i, _i, _vp], _i),
    "sis_stem_conv_wgrad_workspace_bytes": ([_i, _i, _i], _i64),
    "sis_stem_conv_wgrad": ([_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_weight_std_pack_plan": ([_i] * 4 + [_vp] * 5, _i),
    "sis_weight_std_pack_multi": ([_vp, _i, _i, _f, _vp], _i),
    "sis_weight_std_bwd_multi": ([_vp, _vp, _vp, _vp, _i, _vp], _i),
    "sis_conv1x1_bf16_wgrad_supported": ([_i] * 4 + [_i64], _i),
    "sis_conv1x1_bf16_wgrad": ([_vp, _i, _vp, _vp] + [_i] * 4 + [_vp, _i64, _vp], _i),
    "sis_conv1x1_bf16_wgrad_multi": ([_vp, _i, _vp, _vp] + [_i] * 5 + [_vp, _i64, _vp], _i),
    "sis_dconv3x3": ([_vp] * 4 + [_i] * 6 + [_vp], _i),
    "sis_dconv3x3_adjoint": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_dconv3x3_wgrad_workspace_floats": ([_i] * 6, _i64),
    "sis_dconv3x3_wgrad": ([_vp] * 4 + [_i64] + [_i] * 7 + [_vp], _i),
    "sis_channel_sum": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "sis_pixel_shuffle2": ([_vp] * 3 + [_i] * 4 + [_i64, _i, _vp], _i),
    "sis_transpose2d": ([_vp, _vp, _i, _i, _vp], _i),
    "sis_bn_drop_bwd_workspace_floats": ([_i] * 3, _i64),
    "sis_bn_drop_fwd": ([_vp, _i64] + [_vp] * 5 + [_i] * 4 + [_f, _vp, _i, _f, _vp, _vp], _i),
    "sis_bn_drop_bwd": ([_vp] * 4 + [_i64] + [_vp] * 6 + [_f, _vp, _i, _i, _i, _vp], _i),
    "sis_weighted_ce_workspace_floats": ([], _i),
    "sis_weighted_ce_fwd": ([_vp] * 6 + [_i] * 3 + [_vp], _i),
    "sis_weighted_ce_bwd": ([_vp] * 6 + [_i] * 3 + [_vp], _i),
    "sis_adam_chunk_elems": ([], _i),
    "sis_adam_clip_step": ([_vp, _i, _vp, _vp, _vp, _vp], _i),
    "sis_pixel_ensemble_project": ([_vp, _i, _i, _i, _vp], _i),
    "sis_pixel_ensemble_head": ([_vp, _vp, _i] + [_vp] * 10 + [_i] * 5 + [_vp], _i),
    "sis_pe_train_workspace_bytes": ([_i] * 4, _i64),
    "sis_pe_train_gather": ([_vp, _vp, _i, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_pe_train_l1_forward": ([_vp] * 4 + [_i] * 3 + [_vp], _i),
    "sis_pe_train_tail": ([_vp] * 9 + [_i] * 3 + [_vp], _i),
    "sis_pe_train_l1_wgrad": ([_vp] * 5 + [_i] * 3 + [_vp], _i),
    "sis_skm_state_doubles": ([], _i),
    "sis_skm_gather": ([_vp, _vp, _vp, _i64, _i, _i, _i, _vp], _i),
    "sis_skm_loop": ([_vp] * 5 + [_i] * 4 + [_d, _i, _d, _i64, _vp], _i),
    "sis_skm_label_workspace_doubles": ([_i64], _i64),
    "sis_skm_label": ([_vp] * 5 + [_i] * 4 + [_vp], _i),
    "sis_assemble_vote": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "sis_confusion_matrix": ([_vp, _vp, _vp, _vp, _i64, _i, _vp], _i),
    "sis_color_to_class": ([_vp, _vp, _i64, _i, _vp, _vp, _i, _vp], _i),
    "sis_contour_workspace_bytes": ([_i, _i], _i64),
    "sis_remove_small_contours": ([_vp, _vp, _vp, _i64, _i, _i, _i, _f, _i, _i, _vp], _i),
    "sis_cluster_segment_workspace_bytes": ([_i] * 5, _i64),
    "sis_cluster_segment": ([_vp] * 5 + [_i, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp], _i),
    "sis_augment_warp": ([_vp] * 9 + [_i64] + [_i] * 8 + [_vp], _i),
    "sis_elastic_field": ([_vp] * 7 + [_i, _i, _i, _vp], _i),
    "sis_enc_conv3x3_s2_supported": ([_i] * 4, _i),
    "sis_enc_conv3x3_s2_packed_floats": ([_i] * 3, _i64),
    "sis_enc_conv3x3_s2_pack": ([_vp] * 3 + [_i, _i, _vp], _i),
    "sis_enc_conv3x3_s2": ([_vp] * 8 + [_i] * 5 + [_vp], _i),
    "sis_enc_stem_supported": ([_i] * 4, _i),
    "sis_enc_stem": ([_vp] * 10 + [_i] * 5 + [_vp], _i),
    "sis_enc_block_tail_supported": ([_i] * 2, _i),
    "sis_enc_block_tail_tiles": ([_i], _i),
    "sis_enc_block_tail_workspace_floats": ([_i] * 3, _i64),
    "sis_enc_block_tail": ([_vp] * 10 + [_i] * 3 + [_vp], _i),
    "sis_enc_latent_heads_supported": ([_i] * 2, _i),
    "sis_enc_latent_heads": ([_vp, _vp] + [_i] * 6 + [_vp], _i),
    "sis_gan_image_batch": ([_vp, _vp, _vp, _i64, _i, _i, _vp], _i),
    "sis_phase_split_supported": ([_i] * 2, _i),
    "sis_phase_split": ([_vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_phase_merge": ([_vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_down_weight_compose_supported": ([_i] * 2, _i),
    "sis_down_weight_compose": ([_vp, _vp, _vp, _i, _i, _f, _i, _i, _vp], _i),
    "sis_down_weight_compose_adjoint": ([_vp, _vp, _vp, _i, _i, _f, _i, _i, _vp], _i),
    "sis_png_capacity": ([_i, _i], _i64),
    "sis_png_encode_pairs_workspace_bytes": ([_i, _i], _i64),
    "sis_png_encode_pairs": ([_vp] * 4 + [_i] * 4 + [_i64, ctypes.c_uint32, _vp, _i64, _vp], _i),
    "sis_psnr_ssim_tile": ([], _i),
    "sis_psnr_ssim_workspace_bytes": ([_i] * 4, _i64),
    "sis_psnr_ssim": ([_vp] * 5 + [_i] * 5 + [_f, _i, _vp, _i64, _vp], _i),
    "sis_autoencoder_batch": ([_vp] * 8 + [_i64, _i, _i, _vp], _i),
    "sis_label_regions_workspace_bytes": ([_i, _i, _i], _i64),
    "sis_label_regions": ([_vp] * 7 + [_i] * 5 + [_vp, _i64, _vp], _i),
    "sis_page_regions_workspace_bytes": ([_i, _i, _i], _i64),
    "sis_page_regions": ([_vp] * 5 + [_i] * 4 + [ctypes.c_uint32, _i, _i, _vp, _i64, _vp], _i),
    "sis_page_render": ([_vp] * 6 + [_i, _vp, _vp, _vp, _vp, _i, _vp] + [_i] * 5 + [_vp], _i),
    "sis_page_crops": ([_vp, _i64, _vp, _i, _vp, _i, _vp] + [_i] * 4 + [_vp], _i),
    "sis_scan_reduce": ([_vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_scan_resample_workspace_bytes": ([_i] * 4, _i64),
    "sis_scan_resample": ([_vp, _vp] + [_i] * 4 + [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i64, _vp], _i),
    "sis_scan_patches": ([_vp, _vp, _vp] + [_i] * 4 + [_vp], _i),
    "sis_scan_content_box_workspace_bytes": ([_i, _i], _i64),
    "sis_scan_content_box": ([_vp] * 4 + [_i, _vp] + [_i] * 4 + [_vp, _i64, _vp], _i),
    "sis_seg_eval_workspace_bytes": ([_i] * 4, _i64),
    "sis_seg_eval": ([_vp] * 4 + [_i, _vp] + [_i] * 6 + [_vp], _i),
}


def exported_symbols():
    """Every symbol include/sis_hip.h declares (checked by the CPU test-suite)."""
    return sorted(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libsis_hip.so is not built ({LIB_PATH}); run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C synthesis-in-style_amd/csrc`.  There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


_prof = None


def set_profiler(records):
    """bench.py hook: when ``records`` is a list, every kernel launch below is bracketed by HIP events on
    the launch stream and appended as (kernel, algorithmic_flops, algorithmic_bytes, ev0, ev1)."""
    global _prof
    _prof = records


def _launch(kernel, flops, nbytes, call):
    if _prof is None:
        return call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = call()
    e1.record()
    if kernel is None:  # convolutions: the library picks the kernel by shape / alignment and reports its name
        kernel = lib().sis_last_kernel().decode()
    _prof.append((kernel, flops, nbytes, e0, e1))
    return rc


# ---- audit of what does NOT run on this library: every place in the product that hands an operator to
# ATen / MIOpen / hipBLASLt calls ``library_call(site)``.  ``intended=True`` marks the documented exceptions (the two 3-channel
# stems); everything else is a shape the kernels declined and must stay at zero on the BASELINE configs --
# bench.py reports both counters and fails on a non-zero fallback count.
LIBRARY_CALLS = collections.Counter()
_LIBRARY_STRICT = os.environ.get("SIS_NO_LIBRARY_FALLBACK", "0") == "1"


def library_call(site, intended=False):
    LIBRARY_CALLS[("intended:" if intended else "fallback:") + site] += 1
    if _LIBRARY_STRICT and not intended:
        raise RuntimeError(f"SIS_NO_LIBRARY_FALLBACK=1: {site} fell back to the ROCm libraries")


def library_calls(reset=False):
    """{"intended": {site: n}, "fallback": {site: n}} since the last reset."""
    out = {"intended": {}, "fallback": {}}
    for key, n in LIBRARY_CALLS.items():
        kind, site = key.split(":", 1)
        out[kind][site] = n
    if reset:
        LIBRARY_CALLS.clear()
    return out


_own_kernels = None


# ---------------------------------------------------------------------------------------------------- weight stamps
# State derived from a parameter (packed weight images, folded BatchNorms, bf16 copies, tables that hold addresses inside
# them) is current while the parameter's stamp has not moved.  ``_version`` moves with every write autograd
# sees; a write it cannot see (a kernel of this library given ``data_ptr()``, a ``.data`` idiom) is reported by
# ``mark_written``, which the fused optimizers call for their device steps.
RAW_UPDATES = "_sis_raw_updates"


def weight_stamp(t, raw=True):
    """(data_ptr, _version, raw-update counter) of a tensor: equal stamps mean the same storage, not written in between by
    anything that moves ``_version`` or calls ``mark_written``.  ``raw=False`` leaves the counter out (a copy that the raw
    writer itself keeps current)."""
    return (t.data_ptr(), t._version, getattr(t, RAW_UPDATES, 0) if raw else 0)


def mark_written(*targets):
    """Tell the modules that cache state derived from these tensors that their values were changed by a write autograd
    cannot see (``p.data.mul_()``, ``_foreach`` ops on ``.data`` lists, a kernel handed ``p.data_ptr()``, a NumPy view).
    ``targets``: tensors, modules (all their parameters and buffers) or iterables of either.  The mark lives on the tensor
    OBJECT: pass the parameter itself, not ``p.data`` or ``p.detach()``, which are new objects."""
    for target in targets:
        if isinstance(target, torch.Tensor):
            setattr(target, RAW_UPDATES, getattr(target, RAW_UPDATES, 0) + 1)
        elif isinstance(target, torch.nn.Module):
            mark_written(*target.parameters(), *target.buffers())
        else:
            mark_written(*target)


# ---------------------------------------------------------------------------------------------------- side streams
# HIP maps streams onto a handful of hardware queues (4 on this stack), and two streams on ONE queue run their kernels one after
# the other.  Which pool stream lands beside the default stream's queue depends on what else created streams first: after an RCCL
# communicator exists, the FIRST stream torch hands out shares the default stream's queue (tools/stream_probe.py: every fourth
# one does) -- the generator's ToRGB chain then ran behind the convolutions instead of beside them (synthesis 14.29 -> 14.49 ms per
# step, tools/rccl_alive_cost.py), and a gradient exchange on such a stream would not overlap the backward at all.  So a side
# stream is CHOSEN: candidates are probed with a pair of spin kernels and the first that really runs beside its partner is kept.
_SIDE_STREAM_REJECTS = []   # candidates found on the partner's queue: kept alive so that the pool moves on
_SIDE_STREAM_LOG = []       # (device index, candidates tried, ratio of the chosen one): bench.py / tests read it


def _spin_pair_ms(main, cand, cycles):
    device = main.device
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(main):
        e0.record(main)
        if cand is not None:
            cand.wait_event(e0)
        torch.cuda._sleep(cycles)
        if cand is not None:
            with torch.cuda.stream(cand):
                torch.cuda._sleep(cycles)
            main.wait_stream(cand)
        e1.record(main)
    torch.cuda.synchronize(device)
    return e0.elapsed_time(e1)


def runs_beside(main, cand, cycles=2_000_000):
    """True when kernels on ``cand`` run concurrently with kernels on ``main`` (two spin kernels take the time of one)."""
    alone = min(_spin_pair_ms(main, None, cycles) for _ in range(2))
    both = min(_spin_pair_ms(main, cand, cycles) for _ in range(2))
    return both < 1.5 * alone, both / max(alone, 1e-6)


def side_stream(device, beside=None, tries=8):
    """A stream of torch's pool whose kernels run CONCURRENTLY with those of ``beside`` (default: the current stream of
    ``device``).  SIS_STREAM_PROBE=0, or a capture in progress: the first pool stream, unprobed."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("side_stream: a HIP device is required")
    if os.environ.get("SIS_STREAM_PROBE", "1") == "0" or torch.cuda.is_current_stream_capturing():
        return torch.cuda.Stream(device=device)
    main = beside if beside is not None else torch.cuda.current_stream(device)
    cand, ratio = None, None
    for n in range(1, tries + 1):
        cand = torch.cuda.Stream(device=device)
        ok, ratio = runs_beside(main, cand)
        if ok:
            _SIDE_STREAM_LOG.append((device.index, n, round(ratio, 2)))
            return cand
        _SIDE_STREAM_REJECTS.append(cand)
    import warnings
    warnings.warn(f"sis_hip.side_stream: none of {tries} pool streams ran beside the current stream (last ratio {ratio:.2f}); "
                  f"side-stream work will run serially")
    _SIDE_STREAM_LOG.append((device.index, tries, round(ratio, 2)))
    return cand


def own_kernel_names():
    """Names of every ``__global__`` function of csrc/*.hip and csrc/*.h (the library's own device symbols; kernels also live
    in headers a .hip file includes), for classifying profiler records into own / vendor-library kernels."""
    global _own_kernels
    if _own_kernels is None:
        import glob
        import re
        names = set()
        csrc = os.path.join(os.path.dirname(_HERE), "csrc")
        for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
            with open(path) as f:
                text = f.read()
            for m in re.finditer(r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(?:__attribute__\s*\(\(.*?\)\)\s*)?(?:static\s+)?void\s+"
                                 r"(?:__launch_bounds__\s*\([^)]*\)\s*)?([A-Za-z_]\w*)\s*\(", text):
                names.add(m.group(1))
        _own_kernels = frozenset(names)
    return _own_kernels


def is_own_kernel(profiler_name):
    import re
    return any(tok in own_kernel_names() for tok in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", profiler_name))


def _check(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name} failed: {lib().sis_last_error().decode()}")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_device(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")  # same text as the reference CHECK_CUDA


def dtype_code(t):
    try:
        return _DTYPE_CODE[t.dtype]
    except KeyError:
        raise RuntimeError(f"unsupported dtype {t.dtype} (float32/float64/float16/bfloat16)") from None


# ------------------------------------------------------------------------------------------ K1


def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """Same argument order as the reference pybind entry (fused_bias_act.cpp:11-21); empty tensors
    mean "absent" (fused_bias_act_kernel.cu:62-63)."""
    require_device(input, "input")
    require_device(bias, "bias")
    x = input.contiguous()
    b = bias.contiguous() if bias.numel() else None
    r = refer.contiguous() if refer.numel() else None
    if b is not None and b.dtype != x.dtype:
        b = b.to(x.dtype)
    if r is not None:
        require_device(r, "refer")
        if r.dtype != x.dtype:
            r = r.to(x.dtype)
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(lib().sis_fused_bias_act(_ptr(out), _ptr(x), _ptr(b), _ptr(r), dtype_code(x), x.numel(), step_b,
                                        b.numel() if b is not None else 0, int(act), int(grad), float(alpha),
                                        float(scale), _stream()), "sis_fused_bias_act")
    return out


# ------------------------------------------------------------------------------------------ K2


def upfirdn2d_out_size(in_size, up, down, pad0, pad1, k):
    return (in_size * up + pad0 + pad1 - k + down) // down


def upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """Same signature as the reference pybind entry (upfirdn2d.cpp:12-23): input
    [major, in_h, in_w, minor], kernel [kh, kw] -> [major, out_h, out_w, minor]."""
    require_device(input, "input")
    require_device(kernel, "kernel")
    x = input.contiguous()
    k = kernel.contiguous()
    if k.dtype != x.dtype:
        k = k.to(x.dtype)
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h = upfirdn2d_out_size(in_h, up_y, down_y, pad_y0, pad_y1, kh)
    out_w = upfirdn2d_out_size(in_w, up_x, down_x, pad_x0, pad_x1, kw)
    if out_h < 0 or out_w < 0:
        raise RuntimeError(f"upfirdn2d: negative output size {out_h}x{out_w}")
    out = torch.empty((major, out_h, out_w, minor), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_upfirdn2d(_ptr(out), _ptr(x), _ptr(k), dtype_code(x), major, in_h, in_w, minor, kh, kw,
                                   up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, _stream()),
               "sis_upfirdn2d")
    return out


# ------------------------------------------------------------------------------ generator blocks


def _f32(t, name):
    require_device(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: the generator kernels are float32, got {t.dtype}")
    return t.contiguous()


def pixel_norm(x):
    x = _f32(x, "input")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(lib().sis_pixel_norm(_ptr(out), _ptr(x), x.shape[0], x.shape[1], _stream()), "sis_pixel_norm")
    return out


def equal_linear(x, weight, bias, scale, lr_mul, activation, row_stride=None, batch=None):
    """x is [B, in] (or any tensor whose rows are ``row_stride`` floats apart, e.g. latent[:, i])."""
    require_device(x, "input")
    w = _f32(weight, "weight")
    b = _f32(bias, "bias") if bias is not None else None
    if row_stride is None:
        x = _f32(x, "input")
        row_stride, batch = x.shape[1], x.shape[0]
    out = torch.empty((batch, w.shape[0]), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib().sis_equal_linear(_ptr(out), _ptr(x), row_stride, _ptr(w), _ptr(b), batch, w.shape[1], w.shape[0],
                                      float(scale), float(lr_mul), int(bool(activation)), _stream()),
               "sis_equal_linear")
    return out


def head_gemm_tile():
    """Output features per workgroup of the batched modulation / demodulation launches (their tables count blocks in it)."""
    return int(lib().sis_head_gemm_tile())


def modulation_batch(out_flat, latent, table, n_layers, total_blocks, scale):
    """latent [B, n_latent, dim] -> every layer's style vector, written into ``out_flat`` at the table's offsets."""
    b, n_latent, dim = latent.shape
    with torch.cuda.device(latent.device):
        _check(lib().sis_modulation_batch(_ptr(out_flat), _ptr(latent), _ptr(table), n_layers, total_blocks, b, n_latent,
                                          dim, float(scale), _stream()), "sis_modulation_batch")


def demod_batch(dscale_flat, s_flat, table, n_layers, total_blocks, batch):
    with torch.cuda.device(s_flat.device):
        _check(lib().sis_demod_batch(_ptr(dscale_flat), _ptr(s_flat), _ptr(table), n_layers, total_blocks, batch,
                                     _stream()), "sis_demod_batch")


def truncate(w, mean, psi):
    w = _f32(w, "style")
    mean = _f32(mean, "truncation_latent").reshape(-1)
    dim = w.shape[-1]
    if mean.numel() != dim:
        raise RuntimeError("truncation_latent must hold one latent vector")
    out = torch.empty_like(w)
    with torch.cuda.device(w.device):
        _check(lib().sis_truncate(_ptr(out), _ptr(w), _ptr(mean), float(psi), w.numel() // dim, dim, _stream()),
               "sis_truncate")
    return out


def modconv_prepack(weight):
    """weight: ModulatedConv2d.weight [1, Cout, Cin, k, k] -> (wpk [Cin, k*k, Cout], wsq [Cout, Cin])."""
    w = _f32(weight, "weight")
    _, cout, cin, k, _ = w.shape
    wpk = torch.empty((cin, k * k, cout), dtype=torch.float32, device=w.device)
    wsq = torch.empty((cout, cin), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(_launch("modconv_prepack", 0.0, 4.0 * (w.numel() + wpk.numel() + wsq.numel()),
                       lambda: lib().sis_modconv_prepack(_ptr(wpk), _ptr(wsq), _ptr(w), cout, cin, k, _stream())), "sis_modconv_prepack")
    return wpk, wsq


def _prepack_winograd(form, weight, lead, trail):
    """[1, Cout, Cin, 3, 3] -> the transformed weights of a Winograd form, [Cin, *lead, Cout, *trail], through its prepack entry."""
    w = _f32(weight, "weight")
    _, cout, cin, k, _ = w.shape
    if k != 3:
        raise RuntimeError("the Winograd transform is for 3x3 kernels")
    u = torch.empty((cin,) + lead + (cout,) + trail, dtype=torch.float32, device=w.device)
    symbol = f"sis_modconv_prepack_{form}"
    with torch.cuda.device(w.device):
        _check(_launch(symbol[4:], 0.0, 4.0 * (w.numel() + u.numel()),
                       lambda: getattr(lib(), symbol)(_ptr(u), _ptr(w), cout, cin, _stream())), symbol)
    return u


def modconv_prepack_wino(weight):
    """[1, Cout, Cin, 3, 3] -> Winograd F(2x2,3x3) transformed weights [Cin, 16, Cout]."""
    return _prepack_winograd("wino", weight, (16,), ())


def _wino512_eligible(form, cin, cout, h, w):
    return bool(getattr(lib(), f"sis_modconv_{form}_eligible")(int(cin), int(cout), int(h), int(w)))


def modconv_prepack_wino24(weight):
    """[1, Cout, Cin, 3, 3] -> Winograd F(2x4,3x3) transformed weights G2 g G4^T, [Cin, 2 column halves, 3, Cout, 4]."""
    return _prepack_winograd("wino24", weight, (2, 3), (4,))


def modconv_wino24_eligible(cin, cout, h, w):
    """True when the F(2x4,3x3) kernel takes a stride-1 3x3 layer of this shape; the batch size plays no part."""
    return _wino512_eligible("wino24", cin, cout, h, w)


def modconv_prepack_wino44(weight):
    """[1, Cout, Cin, 3, 3] -> Winograd F(4x4,3x3) transformed weights G4 g G4^T, [Cin, 9 rows, Cout, 4] (csrc/modconv_wino44.h)."""
    return _prepack_winograd("wino44", weight, (9,), (4,))


def modconv_wino44_eligible(cin, cout, h, w):
    """True when the F(4x4,3x3) kernel takes a stride-1 3x3 layer of this shape; the batch size plays no part."""
    return _wino512_eligible("wino44", cin, cout, h, w)


# The Winograd forms on 512-pixel tiles, by precedence: (plain symbol, rgb symbol, factor on the direct-form FLOP count).  bench.py
# prices a kernel named "...wino..." at 16/36 of the recorded count: 9/16 x 16/36 = 36/144 and 3/4 x 16/36 = 24/72 are what these run.
_WINO512 = {"wino44": ("sis_modconv2d_wino44", "sis_modconv2d_wino44_rgb", 0.5625),
            "wino24": ("sis_modconv2d_wino24", "sis_modconv2d_wino24_rgb", 0.75)}


BF16_KERNEL = "modconv_bf16_kernel"


def modconv_bf16_eligible(cin, cout, h, w):
    """True when the bf16 matrix-core kernel takes a stride-1 3x3 layer of this shape; the batch size plays no part."""
    return bool(lib().sis_modconv_bf16_eligible(int(cin), int(cout), int(h), int(w)))


def modconv_prepack_bf16(weight):
    """[1, Cout, Cin, 3, 3] -> the bf16 weight image of the bf16 modulated convolution (the raw parameter rounded once to
    nearest even, in the kernel's private tile order), a flat bfloat16 tensor."""
    w = _f32(weight, "weight")
    _, cout, cin, k, _ = w.shape
    if k != 3:
        raise RuntimeError("the bf16 modulated convolution is for 3x3 kernels")
    n = lib().sis_modconv_bf16_packed_elems(cin, cout)
    if n <= 0:
        raise RuntimeError(f"modconv_prepack_bf16: no bf16 weight image for {cin} -> {cout} channels")
    packed = torch.empty((n,), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        _check(_launch("modconv_prepack_bf16", 0.0, 4.0 * w.numel() + 2.0 * packed.numel(),
                       lambda: lib().sis_modconv_prepack_bf16(_ptr(packed), _ptr(w), cout, cin, _stream())), "sis_modconv_prepack_bf16")
    return packed


def conv3x3_supported(x, weight, dilation=1):
    """True when the plain Winograd path takes this layer in both directions (forward and data gradient): 3x3
    kernel, float32 NCHW; a dilation d is run as d*d independent convolutions of the stride-d sub-images, so the
    constraints (W % 4 == 0, H % 2 == 0, channels % 8 == 0, tile plan fits the LDS) apply to [B*d*d, C, H/d, W/d]."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and weight.dim() == 4
            and tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] == x.shape[1]):
        return False
    b, _, h, w = x.shape
    d = int(dilation)
    if d < 1 or h % d or w % d:
        return False
    return conv3x3_shape_supported(b * d * d, weight.shape[1], weight.shape[0], h // d, w // d)


def conv3x3_shape_supported(batch, cin, cout, h, w):
    """``conv3x3_supported`` for a float32 device tensor [batch, cin, h, w] and a [cout, cin, 3, 3] weight that need not exist yet
    (``networks.hip_conv.down_conv3x3`` asks for the phase-split form of its operands)."""
    if cout % 8 or cin % 8:
        return False
    key = (int(batch), int(cin), int(cout), int(h), int(w))
    hit = _conv3x3_ok.get(key)
    if hit is None:
        hit = bool(lib().sis_conv3x3_eligible(*key)) and bool(lib().sis_conv3x3_eligible(key[0], cout, cin, key[3], key[4]))
        _conv3x3_ok[key] = hit
    return hit


_conv3x3_ok = {}


def conv3x3_prepack(weight, adjoint=False):
    """[Cout, Cin, 3, 3] -> Winograd-transformed weights of the forward convolution, or (adjoint) of the convolution
    that takes dL/dy to dL/dx."""
    w = _f32(weight, "weight")
    cout_w, cin_w = w.shape[0], w.shape[1]
    cout, cin = (cin_w, cout_w) if adjoint else (cout_w, cin_w)
    u = torch.empty((cin, 16, cout), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib().sis_conv3x3_prepack(_ptr(u), _ptr(w), cout, cin, int(bool(adjoint)), _stream()), "sis_conv3x3_prepack")
    return u


def conv3x3_prepack_both(weight):
    """(forward image, adjoint image) of ``conv3x3_prepack`` from one launch."""
    w = _f32(weight, "weight")
    cout, cin = w.shape[0], w.shape[1]
    u = torch.empty((cin, 16, cout), dtype=torch.float32, device=w.device)
    ua = torch.empty((cout, 16, cin), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib().sis_conv3x3_prepack_both(_ptr(u), _ptr(ua), _ptr(w), cout, cin, _stream()), "sis_conv3x3_prepack_both")
    return u, ua


class WinogradPackBank:
    """Forward and adjoint Winograd images of a list of float32 3x3 weights, refreshed by ONE launch
    (``sis_conv3x3_prepack_multi``).  ``u[i]`` [Cin,16,Cout] / ``u_adjoint[i]`` [Cout,16,Cin] keep their addresses, ``refresh()``
    rewrites their contents from the weights."""

    def __init__(self, weights):
        self.weights = [w for w in weights]
        dev = self.weights[0].device
        self.u, self.u_adjoint, rows, block = [], [], [], 0
        for w in self.weights:
            if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
                raise RuntimeError("WinogradPackBank: contiguous float32 [Cout, Cin, 3, 3] weights only")
            cout, cin = w.shape[0], w.shape[1]
            self.u.append(torch.empty((cin, 16, cout), dtype=torch.float32, device=dev))
            self.u_adjoint.append(torch.empty((cout, 16, cin), dtype=torch.float32, device=dev))
            rows.append([w.data_ptr(), self.u[-1].data_ptr(), self.u_adjoint[-1].data_ptr(), cout, cin, block])
            block += -(-cout * cin // 256)
        self.total_blocks = block
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.source_ptrs = [w.data_ptr() for w in self.weights]

    def current(self):
        return all(w.data_ptr() == ptr for w, ptr in zip(self.weights, self.source_ptrs))

    def refresh(self):
        with torch.cuda.device(self.table.device):
            _check(lib().sis_conv3x3_prepack_multi(_ptr(self.table), len(self.weights), self.total_blocks, _stream()),
                   "sis_conv3x3_prepack_multi")


def conv3x3(x, u):
    """Stride-1, padding-1 3x3 convolution of x [B,Cin,H,W] with prepacked weights u [Cin,16,Cout]."""
    x = _f32(x, "input")
    batch, cin, h, w = x.shape
    if u.shape[0] != cin:
        raise RuntimeError(f"prepacked weights are for {u.shape[0]} input channels, input has {cin}")
    cout = u.shape[2]
    out = torch.empty((batch, cout, h, w), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device)
    with torch.cuda.device(x.device):
        _check(_launch(None, 2.0 * batch * cout * cin * 9 * h * w, 4.0 * (x.numel() + out.numel() + u.numel()),
                       lambda: lib().sis_conv3x3(_ptr(out), _ptr(x), _ptr(u), batch, cin, cout, h, w, _ptr(ws), ws.numel(),
                                                 _stream())), "sis_conv3x3")
    return out


def conv3x3_wgrad_supported(batch, cin, cout, h, w, min_work=0.0):
    """Capability (tile plan: channels % 64, even H / W, whole 8-tile chunks, workspace).  No size policy any more (``min_work`` =
    multiply-accumulates per tap below which the library would keep the layer): since the round-2 loop and the one-round split-K
    plan the kernel wins from 5e6 upwards (tools/bench_wgrad_small.py: 5x64->64 @16^2 0.025 vs 0.030 ms, 16x128->128 @32^2 0.056 vs
    0.079) and loses 14 us on 512-channel 4^2 / 8^2 maps (0.033 vs 0.019 ms) -- where the library's kernel adds its K slices with
    atomics and returns different bits from run to run (tools/check_conv_determinism.py); this one is deterministic."""
    if float(batch) * h * w * cin * cout < min_work:
        return False
    return bool(lib().sis_conv3x3_wgrad_eligible(batch, cin, cout, h, w, WORKSPACE_BYTES))


def conv3x3_wgrad(x, grad_output, for_param=None, defer=False):
    """dL/dw [Cout,Cin,3,3] of a stride-1, padding-1 3x3 convolution from its input x [B,Cin,H,W] and dL/dy.  ``for_param``: storage
    address of the parameter the result is the gradient of (``grad_out``).  ``defer``: as ``conv_bf16_wgrad``."""
    x = _f32(x, "input")
    gy = _f32(grad_output, "grad_output")
    batch, cin, h, w = x.shape
    cout = gy.shape[1]
    dw = grad_out(for_param, (cout, cin, 3, 3), torch.float32, x.device)
    if defer and _flush_at_end():
        _defer_conv_wgrad(CONV_WGRAD_F32_3X3, x, gy, dw, (batch, cin, cout, h, w))
    else:
        _launch_conv_wgrads(CONV_WGRAD_F32_3X3, (batch, cin, cout, h, w), dw.dtype, x.device, [(x.data_ptr(), gy.data_ptr(), dw.data_ptr())],
                            4.0 * (x.numel() + gy.numel() + dw.numel()))
    return dw


def modconv_demod(s, wsq, scale, demodulate):
    s = _f32(s, "style")
    cout, cin = wsq.shape
    out = torch.empty((s.shape[0], cout), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        _check(lib().sis_modconv_demod(_ptr(out), _ptr(s), _ptr(wsq), s.shape[0], cin, cout, float(scale),
                                       int(bool(demodulate)), _stream()), "sis_modconv_demod")
    return out


# ---- gradient arena: where a parameter's gradient is WRITTEN.  autograd keeps the tensor it is handed for a parameter without a
# gradient, so a weight-gradient kernel that writes into a fresh view of the parameter's slice of the data-parallel wrap's flat
# fp32 buckets (training/grad_exchange.py) puts the gradient where the exchange and the fused SGD read it, with no gather copy.
# ``grad_arena_register`` maps a parameter's storage address to its slice; the bindings allocate through ``grad_out(key, ...)``.
_GRAD_ARENA = {}   # parameter data_ptr -> [weakref to the parameter, flat fp32 buffer, element offset, numel, owner id, handed out]


def grad_arena_register(owner, params, flats, offsets):
    """``params[i]``'s gradient lives at ``flats[i][offsets[i] : offsets[i] + params[i].numel()]`` (fp32, contiguous)."""
    for prm, flat, off in zip(params, flats, offsets):
        _GRAD_ARENA[prm.data_ptr()] = [weakref.ref(prm), flat, int(off), prm.numel(), id(owner), False]


def grad_arena_reset(owner):
    """End of a backward (the owner's ``_finish``): every slice may be handed out again in the next one."""
    for ent in _GRAD_ARENA.values():
        if ent[4] == id(owner):
            ent[5] = False


def grad_arena_release(owner):
    for key in [k for k, v in _GRAD_ARENA.items() if v[4] == id(owner)]:
        del _GRAD_ARENA[key]


def grad_arena_slot(key):
    """(flat buffer, element offset, numel) registered for the parameter whose storage starts at ``key``, provided that
    parameter is alive, holds NO gradient yet (a second backward before the optimizer step must accumulate: its kernels get
    fresh tensors and autograd adds them) and its slice has not been handed out already in this backward (a parameter used by
    two nodes of the graph: the second kernel may run before autograd has accumulated the first result; it must not write
    over it); None otherwise.  A successful call marks the slice as handed out until ``grad_arena_reset``."""
    ent = _GRAD_ARENA.get(key) if key is not None else None
    if ent is None or ent[5]:
        return None
    prm = ent[0]()
    if prm is None or prm.grad is not None or prm.data_ptr() != key:
        return None
    return ent[1], ent[2], ent[3]


def _grad_arena_take(keys):
    for key in keys:
        _GRAD_ARENA[key][5] = True


def grad_out(key, shape, dtype, device):
    """Result tensor of a weight-gradient kernel for the parameter at storage address ``key`` (None / unknown: a fresh tensor):
    a NEW view of the parameter's arena slice when one is registered, so that autograd takes it as ``.grad`` as it is."""
    slot = grad_arena_slot(key)
    if slot is not None:
        flat, off, numel = slot
        n = 1
        for d in shape:
            n *= int(d)
        if n == numel and dtype == flat.dtype and device == flat.device and (flat.data_ptr() + flat.element_size() * off) % 16 == 0:
            _grad_arena_take([key])
            return flat[off:off + numel].view(shape)
    return torch.empty(shape, dtype=dtype, device=device)


def grad_out_fused(keys, rows, cols, device):
    """One [sum(rows), cols] fp32 result covering SEVERAL parameters (the ViT encoder's query | key | value product): the
    arena view when their slices lie back to back in that order, else a fresh tensor."""
    slots = [grad_arena_slot(k) for k in keys]
    if all(s is not None for s in slots):
        flat, off, _ = slots[0]
        at = off
        ok = flat.dtype == torch.float32 and flat.device == device and (flat.data_ptr() + 4 * off) % 16 == 0
        for (f, o, n), r in zip(slots, rows):
            ok = ok and f is flat and o == at and n == r * cols
            at += n
        if ok:
            _grad_arena_take(keys)
            return flat[off:at].view(sum(rows), cols)
    return torch.empty((sum(rows), cols), dtype=torch.float32, device=device)


# ---- late gradients.  A training step is full of tiny second-stage launches (sums of split-K slabs, of per-workgroup partial rows)
# and same-shape weight-gradient products whose results nothing reads before the optimizer or the gradient exchange.  Inside a
# backward a binding may leave such work to ONE launch per kind at the end of the backward (``flush_deferred``; also run before a
# data-parallel bucket leaves and before the fused optimizer step): its result tensor is handed to autograd now and WRITTEN then.
# THE RULE: that is done only where ``may_complete_late`` says that autograd keeps the tensor and nobody reads it before the
# flush; every call site computes ``defer=`` through it.  Outside a backward nothing is ever queued.
_DEFER = os.environ.get("SIS_DEFER_REDUCES", "1") != "0"        # 0: every reduction where its partial results appear (A/B runs)
_DEFER_WGRAD = os.environ.get("SIS_DEFER_WGRAD", "1") != "0"   # 0: every weight gradient where its operands appear (A/B runs)
_deferred = {"ln": [], "wgrad": {}, "conv": {}}   # wgrad: (tokens, out, in, lda, ldb, device) -> [(grad, x, dw, db addresses, storages)]
#                                                   conv: (kind, *dims, dW dtype, device) -> [(x, dL/dy, dw addresses, storages)], kind in _CONV_WGRADS
_defer_blockers = set()         # ids of wrappers that read a gradient the moment autograd hands it over (torch's DistributedDataParallel)
_defer_wgrad_blockers = set()   # ids of data-parallel wrappers with more than one rank: their buckets leave DURING the backward,
                                # overlapped with it -- a weight gradient held back to its end would put the exchange behind it


def block_deferral(owner, blocked=True):
    """No deferred completion of gradients while ``owner`` lives: for consumers that read ``.grad`` inside the backward."""
    (_defer_blockers.add if blocked else _defer_blockers.discard)(id(owner))
    if blocked:
        weakref.finalize(owner, _defer_blockers.discard, id(owner))


def block_wgrad_deferral(owner, blocked=True):
    (_defer_wgrad_blockers.add if blocked else _defer_wgrad_blockers.discard)(id(owner))


def may_complete_late(params, wgrad=True):
    """The gradients of ``params`` may be written as late as ``flush_deferred``: deferral is switched on and not blocked (``wgrad``:
    for a weight-gradient product, which has a switch and a blocker of its own beside those of the reductions), a backward is
    running with grad mode off, and every parameter is a leaf without a gradient and without hooks
    (``backward_scope.taken_as_is``).  ``params`` may be empty: a call site whose consumer flushes before it reads."""
    return (_DEFER and not _defer_blockers and not (wgrad and (_defer_wgrad_blockers or not _DEFER_WGRAD))
            and backward_scope.taken_as_is(params))


def _flush_at_end():
    """Queues ``flush_deferred`` for the end of the running backward (False outside one).  Jobs still pending from ANOTHER
    backward (one that raised, or the enclosing one of a nested backward) are completed first: they own their storages."""
    return backward_scope.at_end("sis_hip.flush_deferred", lambda: flush_deferred(), first=lambda: flush_deferred())


def _hold(*tensors):
    """What a queued job keeps of its tensors: their storages, not the tensors.  A result tensor that a job referenced would
    reach autograd's AccumulateGrad with a use count of two, and a gradient that is not uniquely referenced is CLONED there --
    before the flush has written it.  The storage keeps the memory alive without counting as a reference to the tensor."""
    return tuple(t.untyped_storage() for t in tensors if t is not None)


def deferred_pending():
    return len(_deferred["ln"]) + sum(len(v) for v in _deferred["wgrad"].values()) + sum(len(v) for v in _deferred["conv"].values())


def deferred_wgrad_pending():
    return any(_deferred["wgrad"].values()) or any(_deferred["conv"].values())


# The convolution weight-gradient families, by the kind tag their jobs are queued under.  Per family: the C entry for n layers of
# one shape, its operand order behind dW ("xg": x, dL/dy; "gx": dL/dy, x), whether it takes a dW dtype code, the flops of one
# layer from the job's dims, and the kernel name for the profiler (None: the library reports it).
CONV_WGRAD_F32_3X3, CONV_WGRAD_F32_1X1, CONV_WGRAD_BF16_3X3, CONV_WGRAD_BF16_1X1 = "f3", "f1", 3, 1
_ConvWgrad = collections.namedtuple("_ConvWgrad", "entry order dw_dtype_code flops kernel")
_CONV_WGRADS = {
    CONV_WGRAD_F32_3X3: _ConvWgrad("sis_conv3x3_wgrad_multi", "xg", False,    # fp32 Winograd (EMANet); dims (b, cin, cout, h, w)
                                   lambda b, cin, cout, h, w: 2.0 * b * cout * cin * 9 * h * w, None),
    CONV_WGRAD_F32_1X1: _ConvWgrad("sis_conv1x1_wgrad_f32_multi", "gx", False,   # fp32 1x1 (EMANet); dims (b, cin, cout, pixels)
                                   lambda b, cin, cout, pixels: 2.0 * b * cout * cin * pixels, "conv1x1_wgrad_f32_kernel"),
    CONV_WGRAD_BF16_3X3: _ConvWgrad("sis_conv_bf16_wgrad_multi", "xg", True,   # dims (b, cin, cout, h, w)
                                    lambda b, cin, cout, h, w: 2.0 * b * cout * cin * 9 * h * w, None),
    CONV_WGRAD_BF16_1X1: _ConvWgrad("sis_conv1x1_bf16_wgrad_multi", "xg", True,   # dims (b, cin, cout, pixels)
                                    lambda b, cin, cout, pixels: 2.0 * b * cout * cin * pixels, None),
}


def _launch_conv_wgrads(kind, dims, dw_dtype, device, jobs, nbytes=0.0, workspace=None):
    """Launches the n >= 1 same-shape layers ``jobs`` = [(x, dL/dy, dW addresses, ...)] of one family: the immediate call of a
    binding (one job) and the flush of the queue take this one path.  ``nbytes``: the profiler's byte figure.  ``workspace``:
    (tensor or None, bytes) where the caller brings its own scratch; else the device's shared one."""
    fam = _CONV_WGRADS[kind]
    n = len(jobs)
    arr = ctypes.c_void_p * n
    xs, gys, dws = (arr(*[j[i] for j in jobs]) for i in range(3))
    if workspace is None:
        ws = _workspace(device)
        workspace = (ws, ws.numel())
    args = ((dws, _DTYPE_CODE[dw_dtype]) if fam.dw_dtype_code else (dws,)) + ((xs, gys) if fam.order == "xg" else (gys, xs)) \
        + (n,) + tuple(dims) + (_ptr(workspace[0]), workspace[1])
    with torch.cuda.device(device):
        _check(_launch(fam.kernel, fam.flops(*dims) * n, nbytes, lambda: getattr(lib(), fam.entry)(*args, _stream())), fam.entry)


def _defer_conv_wgrad(kind, x, grad_output, dw, dims):
    """Queues a convolution's weight gradient (kind "f3": fp32 Winograd 3x3, "f1": fp32 1x1, 3: bf16 3x3, 1: bf16 1x1 -- the keys
    of ``_CONV_WGRADS``) for the batched launch of ``flush_deferred``: layers of one shape (the trunks' repeated bottleneck units)
    share one tile launch and one reduction launch, planned for their joint workgroup count.  ``dw`` is valid after the flush
    only; the caller guarantees that nothing reads it before."""
    key = (kind,) + tuple(dims) + (dw.dtype, x.device)
    _deferred["conv"].setdefault(key, []).append((x.data_ptr(), grad_output.data_ptr(), dw.data_ptr(), _hold(x, grad_output, dw)))


def _flush_conv_wgrads():
    queued, _deferred["conv"] = _deferred["conv"], {}
    for key, jobs in queued.items():
        _launch_conv_wgrads(key[0], key[1:-2], key[-2], key[-1], jobs)


def defer_wgrad_bias(grad, x, dw=None):
    """Queues the weight / bias gradient of a Linear layer (``gemm_bf16_wgrad_bias``'s operands) for the batched launch of
    ``flush_deferred`` -- one pointer-table GEMM per Linear shape for all queued layers, each contracting its whole token axis per
    tile (no split-K slabs, no reduction launches: 2.61 -> 2.02 ms for the twelve blocks of ViT-B at 8 192 tokens,
    tools/bench_wgrad_multi.py).  Returns (dw, db): allocated now, VALID ONLY AFTER THE FLUSH (the caller asked
    ``may_complete_late`` for the layer's parameters).  None outside a backward and when the operands do not qualify (the caller
    then multiplies on the spot)."""
    if not (grad.dim() == 2 and x.dim() == 2 and grad.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
            and grad.stride(1) == 1 and x.stride(1) == 1 and grad.shape[0] == x.shape[0] and grad.stride(0) % 8 == 0
            and x.stride(0) % 8 == 0 and grad.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and grad.shape[1] % 4 == 0
            and x.shape[1] % 4 == 0 and _flush_at_end()):
        return None
    k, m = grad.shape
    n = x.shape[1]
    if dw is None:
        dw = torch.empty((m, n), dtype=torch.float32, device=grad.device)
    elif tuple(dw.shape) != (m, n) or dw.dtype != torch.float32 or not dw.is_contiguous():
        raise RuntimeError("defer_wgrad_bias: dw must be a contiguous float32 [out, in] tensor")
    db = torch.empty(m, dtype=torch.float32, device=grad.device)
    key = (k, m, n, grad.stride(0), x.stride(0), grad.device)
    _deferred["wgrad"].setdefault(key, []).append((grad.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), _hold(grad, x, dw, db)))
    return dw, db


def flush_deferred():
    """Runs every queued reduction (one launch per 32 jobs) and weight gradient (one launch per Linear shape and 16 jobs).
    Cheap when nothing is queued."""
    if _deferred["conv"]:
        _flush_conv_wgrads()
    if _deferred["wgrad"]:
        queued, _deferred["wgrad"] = _deferred["wgrad"], {}
        for key, jobs in queued.items():
            _wgrad_multi_raw([j[:4] for j in jobs], key)
    jobs = _deferred["ln"]
    if jobs:
        _deferred["ln"] = []
        n = len(jobs)
        vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
        with torch.cuda.device(jobs[0][5]):
            _check(lib().sis_layer_norm_param_reduce_multi(vp(*[j[0] for j in jobs]), vp(*[j[1] for j in jobs]), vp(*[j[2] for j in jobs]),
                                                           ci(*[j[3] for j in jobs]), ci(*[j[4] for j in jobs]), n, _stream()),
                   "sis_layer_norm_param_reduce_multi")


WORKSPACE_BYTES = int(os.environ.get("SIS_WORKSPACE_MB", "128")) << 20  # split-K slabs (per device)
_workspaces = {}


def _workspace(device):
    """Per-device scratch for split-K partial sums (stream-ordered reuse: one stream per device at a time)."""
    ws = _workspaces.get(device)
    if ws is None:
        ws = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        _workspaces[device] = ws
    return ws


def _noise_args(noise, batch, h, w):
    if noise is None:
        return None, 0
    noise = _f32(noise, "noise")
    if noise.numel() == h * w:
        return noise, 0
    if noise.numel() == batch * h * w:
        return noise, h * w
    raise RuntimeError(f"noise shape {tuple(noise.shape)} does not broadcast over [{batch}, C, {h}, {w}]")


def _out_or_new(out, shape, device, what):
    """``out``: a caller-provided contiguous float32 result tensor (e.g. a batch slice of a larger one) or None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise RuntimeError(f"{what}: out must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")
    return out


def rgb_part_shape(batch, cout, h, w):
    """Shape of the partial-sum buffer that ``modconv2d(..., rgb=)`` fills and ``rgb_finish`` reads."""
    return (cout // 64, batch, 3, h, w)


def modconv2d(x, wpk, s, dscale, ksize, noise=None, noise_weight=None, bias=None, fuse_act=False, wino_u=None, out=None,
              wino24_u=None, wino24_tiles_per_wg=0, rgb=None, bf16_w=None, wino44_u=None, wino44_tiles_per_wg=0):
    """``bf16_w`` (modconv_prepack_bf16): the layer runs with bf16 operands on the bf16 matrix cores where modconv_bf16_eligible
    says so, whatever the batch (not together with ``rgb``); other shapes take the path they took without it.

    ``wino24_u`` (modconv_prepack_wino24): the layer runs on the F(2x4,3x3) kernel where modconv_wino24_eligible says so,
    whatever the batch; other shapes take the path they took without it.  ``wino24_tiles_per_wg``: tests only.

    ``wino44_u`` (modconv_prepack_wino44): the layer runs on the F(4x4,3x3) kernel where modconv_wino44_eligible says so, ahead
    of ``wino24_u``; an error where it does not (the caller asks first).  ``wino44_tiles_per_wg``: tests only.

    ``rgb`` = (weight [3 * Cout], s_rgb [B, Cout], scale, part): the Winograd kernel that takes the layer (F(4x4,3x3) with
    ``wino44_u``, else F(2x4,3x3)) also leaves the following ToRGB's channel sum in ``part`` (``rgb_part_shape``), in blocks of 64
    channels, for ``rgb_finish``; an error where that kernel does not take the layer.

    ``out``: a caller's contiguous float32 result tensor to write into (tools/bench_gen_bf16.py rotates more outputs than the
    cache holds)."""
    x = _f32(x, "input")
    batch, cin, h, w = x.shape
    cout = wpk.shape[2]
    noise, nbs = _noise_args(noise, batch, h, w)
    out = _out_or_new(out, (batch, cout, h, w), x.device, "modconv2d")
    tail = (_ptr(s), _ptr(dscale), _ptr(noise), nbs, _ptr(noise_weight), _ptr(bias))
    shape, fuse, fast = (batch, cin, cout, h, w), int(bool(fuse_act)), ksize == 3 and batch > 0
    # The entry, chosen once: its C symbol, the factor on the direct-form FLOP count, what it reads besides x (with the element
    # size) and its arguments up to the stream.
    form = None
    if wino44_u is not None:
        if not (fast and modconv_wino44_eligible(cin, cout, h, w)):
            raise RuntimeError(f"modconv2d: wino44_u= needs the F(4x4,3x3) kernel, which does not take {cin} -> {cout} at {h}x{w}")
        form = "wino44"
    elif rgb is not None:
        if wino24_u is None or not fast or not modconv_wino24_eligible(cin, cout, h, w):
            raise RuntimeError(f"modconv2d: rgb= needs the F(2x4,3x3) kernel, which does not take {cin} -> {cout} at {h}x{w}")
        form = "wino24"
    elif bf16_w is not None and fast and modconv_bf16_eligible(cin, cout, h, w):
        form = "bf16"
    elif wino24_u is not None and fast and modconv_wino24_eligible(cin, cout, h, w):
        form = "wino24"
    if form in _WINO512:
        u, tpw = (wino44_u, wino44_tiles_per_wg) if form == "wino44" else (wino24_u, wino24_tiles_per_wg)
        symbol, symbol_rgb, factor = _WINO512[form]
        reads, args = ((u, 4.0),), (_ptr(out), _ptr(x), _ptr(u)) + tail + shape + (fuse, int(tpw))
        if rgb is not None:
            rgb_w, rgb_s, rgb_scale, part = rgb
            rgb_w, rgb_s = _f32(rgb_w, "rgb weight"), _f32(rgb_s, "rgb style")
            if rgb_w.numel() != 3 * cout or tuple(rgb_s.shape) != (batch, cout):
                raise RuntimeError(f"modconv2d: rgb weight {tuple(rgb_w.shape)} / style {tuple(rgb_s.shape)} do not fit 3 x {cout} channels")
            _out_or_new(part, rgb_part_shape(batch, cout, h, w), x.device, "modconv2d rgb part")
            symbol, reads = symbol_rgb, reads + ((part, 4.0),)
            args = (_ptr(out), _ptr(part), _ptr(x), _ptr(u)) + tail + (_ptr(rgb_w), _ptr(rgb_s), float(rgb_scale)) + shape + (fuse, int(tpw))
    elif form == "bf16":
        if bf16_w.dtype != torch.bfloat16 or bf16_w.numel() != lib().sis_modconv_bf16_packed_elems(cin, cout) or not bf16_w.is_contiguous():
            raise RuntimeError(f"modconv2d: bf16_w is not the modconv_prepack_bf16 image of a {cin} -> {cout} layer")
        symbol, factor, reads = "sis_modconv2d_bf16", 1.0, ((bf16_w, 2.0),)
        args = (_ptr(out), _ptr(x), _ptr(bf16_w)) + tail + shape + (fuse,)
    else:   # the general entry: F(2x2,3x3) where ``wino_u`` is given and that kernel takes the shape, else the direct kernels
        ws = _workspace(x.device)
        symbol, factor, reads = "sis_modconv2d", 1.0, ((wpk, 4.0),)
        args = (_ptr(out), _ptr(x), _ptr(wpk)) + tail + shape + (ksize, fuse, _ptr(wino_u), _ptr(ws), ws.numel())
    with torch.cuda.device(x.device):
        _check(_launch(None, factor * 2.0 * batch * cout * cin * ksize * ksize * h * w,
                       4.0 * (x.numel() + out.numel()) + sum(size * t.numel() for t, size in reads),
                       lambda: getattr(lib(), symbol)(*args, _stream())), symbol)
    return out


_UP_FIR = os.environ.get("SIS_UP_FIR", "1") != "0"   # 0: up-convolutions on the 4-phase gather kernel only (A/B runs)


def modconv_prepack_up_fir(weight):
    """[1, Cout, Cin, 3, 3] parameter -> the 16 transformed planes of the fast-FIR up-convolution, [Cin, 8 plane pairs, Cout, 2]."""
    w = _f32(weight, "weight")
    if w.dim() == 5:
        w = w[0]
    cout, cin = w.shape[0], w.shape[1]
    u = torch.empty((cin, 8, cout, 2), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(_launch("modconv_up_fir_prepack", 0.0, 4.0 * (w.numel() + u.numel()),
                       lambda: lib().sis_modconv_up_fir_prepack(_ptr(u), _ptr(w), cout, cin, _stream())), "sis_modconv_up_fir_prepack")
    return u


def modconv2d_up(x, wpk, s, dscale, padded_rows=False, fir_u=None):
    """Transposed stride-2 modulated conv -> [B, Cout, 2H+1, 2W+1].  ``padded_rows=True`` returns the buffer with
    rows padded to 2W+4 floats ([..., 2H+1, 2W+4], first 2W+1 columns meaningful) for sis_blur_noise_act.  ``fir_u``
    (modconv_prepack_up_fir) selects the fast-FIR kernel where it applies (padded rows, maps of 32 x 32 and larger)."""
    x = _f32(x, "input")
    batch, cin, h, w = x.shape
    cout = wpk.shape[2]
    row = 2 * w + 4 if padded_rows else 2 * w + 1
    out = torch.empty((batch, cout, 2 * h + 1, row), dtype=torch.float32, device=x.device)
    if fir_u is not None and _UP_FIR and padded_rows and lib().sis_modconv_up_fir_supported(batch, cin, cout, h, w, row):
        with torch.cuda.device(x.device):
            # (FLOPs recorded in the direct 9-multiplies-per-position count of SURVEY.md 8(d); the kernel executes 25 / 36 of it)
            _check(_launch(None, 2.0 * batch * cout * cin * 9 * h * w, 4.0 * (x.numel() + out.numel() + fir_u.numel()),
                           lambda: lib().sis_modconv2d_up_fir(_ptr(out), _ptr(x), _ptr(fir_u), _ptr(s), _ptr(dscale), batch, cin, cout,
                                                              h, w, row, _stream())), "sis_modconv2d_up_fir")
        return out
    ws = _workspace(x.device)
    with torch.cuda.device(x.device):
        _check(_launch(None, 2.0 * batch * cout * cin * 9 * h * w,
                       4.0 * (x.numel() + out.numel() + wpk.numel()),
                       lambda: lib().sis_modconv2d_up(_ptr(out), _ptr(x), _ptr(wpk), _ptr(s), _ptr(dscale), batch, cin,
                                                      cout, h, w, row, _ptr(ws), ws.numel(), _stream())),
               "sis_modconv2d_up")
    return out


def blur_noise_act(x, taps, pad, noise=None, noise_weight=None, bias=None, fuse_act=False, in_w=None):
    """``in_w``: meaningful width when the rows of ``x`` are padded (x.shape[3] is then the row stride)."""
    x = _f32(x, "input")
    taps = _f32(taps, "kernel")
    batch, ch, ih, row_stride = x.shape
    iw = row_stride if in_w is None else in_w
    kh, kw = taps.shape
    oh, ow = ih + pad[0] + pad[1] - kh + 1, iw + pad[0] + pad[1] - kw + 1
    noise, nbs = _noise_args(noise, batch, oh, ow)
    out = torch.empty((batch, ch, oh, ow), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("blur_rows_kernel", 0.0, 4.0 * (batch * ch * ih * iw + out.numel()),
                       lambda: lib().sis_blur_noise_act(_ptr(out), _ptr(x), _ptr(taps), _ptr(noise), nbs,
                                                        _ptr(noise_weight), _ptr(bias), batch, ch, ih, iw, row_stride,
                                                        kh, kw, pad[0], pad[1], int(bool(fuse_act)), _stream())),
               "sis_blur_noise_act")
    return out


def to_rgb(x, weight, s, bias, scale, skip=None, taps=None, pad=(0, 0)):
    x = _f32(x, "input")
    w = _f32(weight, "weight")
    batch, cin, h, wd = x.shape
    cout = w.numel() // cin
    kh = kw = 0
    if skip is not None:
        skip = _f32(skip, "skip")
        taps = _f32(taps, "kernel")
        kh, kw = taps.shape
    out = torch.empty((batch, cout, h, wd), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("to_rgb_kernel", 0.0, 4.0 * (x.numel() + out.numel() + (skip.numel() if skip is not None else 0)),
                       lambda: lib().sis_to_rgb(_ptr(out), _ptr(x), _ptr(w), _ptr(s), _ptr(bias), _ptr(skip),
                                                _ptr(taps), batch, cin, cout, h, wd, kh, kw, pad[0], pad[1],
                                                float(scale), _stream())), "sis_to_rgb")
    return out


def rgb_finish(part, bias, skip=None, taps=None, pad=(0, 0)):
    """The ToRGB image from the channel-block sums ``part`` [Cout / 64, B, 3, H, W] of ``modconv2d(..., rgb=)``:
    sum over the blocks + bias + upsampled skip (as ``to_rgb``)."""
    part = _f32(part, "part")
    blocks, batch, cout, h, wd = part.shape
    kh = kw = 0
    if skip is not None:
        skip = _f32(skip, "skip")
        taps = _f32(taps, "kernel")
        kh, kw = taps.shape
    out = torch.empty((batch, cout, h, wd), dtype=torch.float32, device=part.device)
    with torch.cuda.device(part.device):
        _check(_launch("rgb_finish_kernel", 0.0, 4.0 * (part.numel() + out.numel() + (skip.numel() if skip is not None else 0)),
                       lambda: lib().sis_rgb_finish(_ptr(out), _ptr(part), _ptr(bias), _ptr(skip), _ptr(taps), batch, blocks, cout,
                                                    h, wd, kh, kw, pad[0], pad[1], _stream())), "sis_rgb_finish")
    return out


# ------------------------------------------------------------------------------ segmentation training


def upsample_ce_fwd(logits, labels, out_size, ignore_index):
    """loss[B] of bilinear(align_corners) + log-softmax + NLL + spatial mean; labels int64 [B, H, W]."""
    x = _f32(logits, "logits")
    require_device(labels, "labels")
    if labels.dtype != torch.int64:
        raise RuntimeError(f"labels must be int64, got {labels.dtype}")
    lab = labels.contiguous()
    b, c, h, w = x.shape
    oh, ow = out_size
    if tuple(lab.shape) != (b, oh, ow):
        raise RuntimeError(f"labels shape {tuple(lab.shape)} != {(b, oh, ow)}")
    L = lib()
    ws = torch.empty(L.sis_upsample_ce_workspace(b, oh, ow), dtype=torch.float32, device=x.device)
    loss = torch.empty(b, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(L.sis_upsample_ce_fwd(_ptr(loss), _ptr(ws), _ptr(x), _ptr(lab), b, c, h, w, oh, ow, int(ignore_index),
                                     _stream()), "sis_upsample_ce_fwd")
    return loss


def upsample_ce_bwd(grad_loss, logits, labels, out_size, ignore_index):
    x = _f32(logits, "logits")
    g = _f32(grad_loss, "grad_loss")
    lab = labels.contiguous()
    b, c, h, w = x.shape
    gx = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(lib().sis_upsample_ce_bwd(_ptr(gx), _ptr(g), _ptr(x), _ptr(lab), b, c, h, w, out_size[0], out_size[1],
                                         int(ignore_index), _stream()), "sis_upsample_ce_bwd")
    return gx


def seg_eval_state(classes, device):
    """Fresh zeroed state of ``seg_eval``: counts int64 [C*C + 2] and sums float64 [1 + 3C] on ``device``."""
    return (torch.zeros(classes * classes + 2, dtype=torch.int64, device=device),
            torch.zeros(1 + 3 * classes, dtype=torch.float64, device=device))


def seg_eval(logits, labels, size=None, counts=None, sums=None):
    """One validation pass over a batch (csrc/seg_eval.h): ``logits`` [B,C,h,w] (float32, or bfloat16 at the size
    of the labels), ``labels`` int64 [B,H,W] or [B,1,H,W]; ``size`` = (H, W), taken from the labels when None.  Where (h, w) !=
    (H, W) the logits are interpolated (bilinear, align_corners) inside the kernel, as ``upsample_ce_fwd`` does.  ACCUMULATES into
    ``counts`` (int64 [C*C + 2]: matrix[label][argmax] row-major, counted, ignored) and ``sums`` (float64 [1 + 3C]: sum of -log
    softmax[label] over the counted pixels, then I_c, P_c, T_c per class) and returns both; fresh zeroed state when None."""
    require_device(logits, "logits")
    require_device(labels, "labels")
    if logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() != 4:
        raise RuntimeError(f"logits must be a float32 or bfloat16 [B, C, h, w] tensor, got {logits.dtype} {tuple(logits.shape)}")
    if labels.dtype != torch.int64:
        raise RuntimeError(f"labels must be int64, got {labels.dtype}")
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    b, c, h, w = logits.shape
    if labels.dim() != 3 or labels.shape[0] != b:
        raise RuntimeError(f"labels must be [B, H, W] or [B, 1, H, W] with B = {b}, got {tuple(labels.shape)}")
    oh, ow = (int(size[0]), int(size[1])) if size is not None else (int(labels.shape[1]), int(labels.shape[2]))
    if tuple(labels.shape[1:]) != (oh, ow):
        raise RuntimeError(f"labels shape {tuple(labels.shape)} != {(b, oh, ow)}")
    x, lab = logits.contiguous(), labels.contiguous()
    if counts is None:
        counts = torch.zeros(c * c + 2, dtype=torch.int64, device=x.device)
    if sums is None:
        sums = torch.zeros(1 + 3 * c, dtype=torch.float64, device=x.device)
    if counts.dtype != torch.int64 or tuple(counts.shape) != (c * c + 2,) or not counts.is_contiguous() or counts.device != x.device:
        raise RuntimeError(f"counts must be a contiguous int64 [{c * c + 2}] tensor on {x.device}, got {counts.dtype} {tuple(counts.shape)}")
    if sums.dtype != torch.float64 or tuple(sums.shape) != (1 + 3 * c,) or not sums.is_contiguous() or sums.device != x.device:
        raise RuntimeError(f"sums must be a contiguous float64 [{1 + 3 * c}] tensor on {x.device}, got {sums.dtype} {tuple(sums.shape)}")
    L = lib()
    ws_bytes = L.sis_seg_eval_workspace_bytes(b, c, oh, ow)
    if ws_bytes <= 0:
        raise RuntimeError(f"seg_eval: {c} classes (2..16) or batch {b}, size {oh} x {ow} out of range")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(L.sis_seg_eval(_ptr(counts), _ptr(sums), _ptr(ws), _ptr(x), _DTYPE_CODE[x.dtype], _ptr(lab), b, c, h, w, oh, ow,
                              _stream()), "sis_seg_eval")
    return counts, sums


def sgd_chunk_elems():
    return lib().sis_sgd_chunk_elems()


def sgd_momentum(table, n_chunks, lrs, wds, momentum, first_step):
    n = len(lrs)
    arr = _f * n
    with torch.cuda.device(table.device):
        _check(lib().sis_sgd_momentum(_ptr(table), n_chunks, arr(*lrs), arr(*wds), n, float(momentum),
                                      int(bool(first_step)), _stream()), "sis_sgd_momentum")


def sgd_momentum_dev(table, n_chunks, hyper):
    """Capturable variant: lr[4], wd[4], momentum are read from the device tensor ``hyper`` (float32[9])."""
    with torch.cuda.device(table.device):
        _check(lib().sis_sgd_momentum_dev(_ptr(table), n_chunks, _ptr(hyper), _stream()), "sis_sgd_momentum_dev")


def ema_update(mu, mu_batch, momentum):
    """In place: mu <- mu*m + mean_b(mu_batch)*(1-m); (1-m) is formed in double like the reference's Python."""
    require_device(mu, "mu")
    mb = _f32(mu_batch, "mu_batch")
    if not mu.is_contiguous() or mu.dtype != torch.float32:
        raise RuntimeError("mu must be a contiguous float32 buffer")
    n = mu.numel()
    with torch.cuda.device(mu.device):
        _check(lib().sis_ema_update(_ptr(mu), _ptr(mb), float(momentum), float(1 - momentum), mb.numel() // n, n,
                                    _stream()), "sis_ema_update")
    return mu


def half_dilation_taps(weight):
    """[4 cout, 4 cin] matrix of a 3x3 convolution whose dilation is half the image side (see include/sis_hip.h)."""
    require_device(weight, "weight")
    w = _f32(weight, "weight")
    cout, cin = w.shape[0], w.shape[1]
    taps = torch.empty((4 * cout, 4 * cin), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib().sis_half_dilation_taps(_ptr(taps), _ptr(w), cout, cin, _stream()), "sis_half_dilation_taps")
    return taps


def half_dilation_taps_bwd(grad_taps, cout, cin, for_param=None):
    g = _f32(grad_taps, "grad_taps")
    dw = grad_out(for_param, (cout, cin, 3, 3), torch.float32, g.device)
    with torch.cuda.device(g.device):
        _check(lib().sis_half_dilation_taps_bwd(_ptr(dw), _ptr(g), cout, cin, _stream()), "sis_half_dilation_taps_bwd")
    return dw


def emau_supported(x, mu):
    """x [b, c, h, w] (or [b, c, n]) float32 on a HIP device, mu [1, c, 64]."""
    if not (x.is_cuda and x.dtype == torch.float32 and mu.dtype == torch.float32 and x.dim() in (3, 4) and mu.dim() == 3):
        return False
    b, c = x.shape[0], x.shape[1]
    n = x.numel() // max(b * c, 1)
    return mu.shape[0] == 1 and mu.shape[1] == c and bool(lib().sis_emau_supported(b, c, n, mu.shape[2]))


def emau_forward(x, mu, stages):
    """The EM rounds + reconstruction of EMAU.forward (networks/ema_net/network.py:229-247) -> (relu(mu z^T) shaped like x,
    mu [b, c, k]); no autograd graph (the reference runs the rounds under no_grad and the reconstruction only sees their
    results)."""
    require_device(x, "x")
    x, m0 = _f32(x, "x"), _f32(mu, "mu")
    b, c = x.shape[0], x.shape[1]
    n, k = x.numel() // (b * c), m0.shape[2]
    out = torch.empty_like(x)
    mu_out = torch.empty((b, c, k), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib().sis_emau_workspace_floats(b, c, n, k), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("emau_kernels", 2.0 * b * c * n * k * (2 * stages + 1), 4.0 * (2 * x.numel() + (2 * stages + 1) * (b * n * k + b * c * k)),
                       lambda: lib().sis_emau_forward(_ptr(out), _ptr(mu_out), _ptr(x), _ptr(m0), _ptr(ws), b, c, n, k, int(stages),
                                                      _stream())), "sis_emau_forward")
    return out, mu_out


# ------------------------------------------------------------------------------ dataset-loop neighbours


def kmeans_assign(x, centres):
    """[B,C,H,W] activations, [K,C] centres -> int64 [B,H,W] nearest-centre ids (FactorCatalog.predict)."""
    x = _f32(x, "input")
    c = _f32(centres, "cluster_centers")
    b, ch, h, w = x.shape
    if c.shape[1] != ch:
        raise RuntimeError(f"centres have {c.shape[1]} channels, activations {ch}")
    labels = torch.empty((b, h, w), dtype=torch.int64, device=x.device)
    ws = torch.empty(lib().sis_kmeans_workspace_ints(b, h * w), dtype=torch.int32, device=x.device)   # list of the pixels the fast pass leaves open
    with torch.cuda.device(x.device):
        _check(_launch("kmeans_assign_kernel", 3.0 * b * ch * h * w * c.shape[0], 4.0 * x.numel() + 8.0 * labels.numel(),
                       lambda: lib().sis_kmeans_assign_ws(_ptr(labels), _ptr(x), _ptr(c), b, ch, h * w, c.shape[0], _ptr(ws), ws.numel(),
                                                          _stream())), "sis_kmeans_assign")
    return labels


def make_image_u8(x):
    """[B,C,H,W] float32 in [-1,1] -> uint8 [B,H,W,C] on the device."""
    x = _f32(x, "image")
    b, ch, h, w = x.shape
    out = torch.empty((b, h, w, ch), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_make_image_u8(_ptr(out), _ptr(x), b, ch, h * w, _stream()), "sis_make_image_u8")
    return out


# ------------------------------------------------------------------------------ spherical k-means fit (csrc/spherical_kmeans.hip)
SKM_KMAX, SKM_BMAX = 32, 256   # centre rows per fit in the centres tensor, label slots per fit in last_labels


def skm_gather(x, idx):
    """[B,C,H,W] activation, int32 [n] rows of partial_flat(x) -> [n,C] unit rows (a zero row stays zero)."""
    x = _f32(x, "X")
    require_device(idx, "idx")
    if idx.dtype != torch.int32:
        raise RuntimeError(f"idx must be int32, got {idx.dtype}")
    idx = idx.contiguous()
    b, ch, h, w = x.shape
    out = torch.empty((idx.numel(), ch), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("skm_gather_kernel", 3.0 * idx.numel() * ch, 8.0 * idx.numel() * ch,
                       lambda: lib().sis_skm_gather(_ptr(out), _ptr(x), _ptr(idx), idx.numel(), b, ch, h * w, _stream())),
               "sis_skm_gather")
    return out


def skm_new_state(ks, device):
    """float64 [len(ks), sis_skm_state_doubles()] start state (zero counts, iteration 0) for fits with ks[i] clusters."""
    state = torch.zeros((len(ks), lib().sis_skm_state_doubles()), dtype=torch.float64)
    state[:, 6] = torch.as_tensor(list(ks), dtype=torch.float64)
    return state.to(device)


def skm_loop(state, centres, last_labels, rows, picks, batch_size, iters, alpha, max_no_improvement, reassignment_ratio,
             max_iterations):
    """Advance every unfinished fit by up to ``iters`` mini-batch iterations, in place (state float64 [F,40], centres float32
    [F,32,C], last_labels int32 [F,256], rows float32 [>= iters*batch_size, C], picks int32 [>= iters, 32])."""
    for t, name, dt in ((state, "state", torch.float64), (centres, "centres", torch.float32), (last_labels, "last_labels", torch.int32),
                        (rows, "rows", torch.float32), (picks, "picks", torch.int32)):
        require_device(t, name)
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {dt} tensor")
    f, _, ch = centres.shape
    if (centres.shape[1] != SKM_KMAX or state.shape != (f, lib().sis_skm_state_doubles()) or last_labels.shape != (f, SKM_BMAX)
            or rows.numel() < iters * batch_size * ch or picks.numel() < iters * 32):
        raise RuntimeError("skm_loop: tensor shapes do not match (F fits, 32 centre rows, iters * batch_size rows, iters * 32 picks)")
    with torch.cuda.device(centres.device):
        _check(_launch("skm_loop_kernel", 2.0 * f * iters * batch_size * ch * SKM_KMAX, 4.0 * f * iters * batch_size * ch * 2,
                       lambda: lib().sis_skm_loop(_ptr(state), _ptr(centres), _ptr(last_labels), _ptr(rows), _ptr(picks), f, ch,
                                                  int(batch_size), int(iters), float(alpha), int(max_no_improvement),
                                                  float(reassignment_ratio), int(max_iterations), _stream())), "sis_skm_loop")


def skm_label(x, centres):
    """[B,C,H,W] activation, [K,C] centres -> (int64 [B*H*W] labels of the unit-normalised pixels, float64 [33] device tensor:
    inertia, then the pixel count of each centre)."""
    x = _f32(x, "X")
    c = _f32(centres, "cluster_centers")
    b, ch, h, w = x.shape
    if c.dim() != 2 or c.shape[1] != ch:
        raise RuntimeError(f"centres {tuple(c.shape)} do not match {ch} channels")
    labels = torch.empty(b * h * w, dtype=torch.int64, device=x.device)
    result = torch.empty(33, dtype=torch.float64, device=x.device)
    ws = torch.empty(lib().sis_skm_label_workspace_doubles(b * h * w), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("skm_label_kernel", 2.0 * b * ch * h * w * 32, 4.0 * x.numel() + 8.0 * labels.numel(),
                       lambda: lib().sis_skm_label(_ptr(labels), _ptr(result), _ptr(ws), _ptr(x), _ptr(c), b, ch, h * w, c.shape[0],
                                                   _stream())), "sis_skm_label")
    return labels, result


# ------------------------------------------------------------------------------ fp32 pointwise convolution (matrix cores, NCHW)


def conv1x1_f32_supported(x, weight):
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
            and x.data_ptr() % 16 == 0
            and bool(lib().sis_conv1x1_f32_supported(weight.shape[1], weight.shape[0], x.shape[2] * x.shape[3])))


def conv1x1_f32(x, weight, bias=None, data_gradient=False):
    """1x1 stride-1 fp32 convolution of x [B,Cin,H,W] with weight [Cout,Cin,1,1] (+ bias), or with ``data_gradient`` the
    gradient w.r.t. the input from x = dL/dy [B,Cout,H,W]."""
    x = _f32(x, "input")
    w = _f32(weight, "weight")
    b, cx, h, wd = x.shape
    cout, cin = w.shape[0], w.shape[1]
    if cx != (cout if data_gradient else cin):
        raise RuntimeError(f"conv1x1_f32: input has {cx} channels, weight is {cout}x{cin}")
    out = torch.empty((b, cin if data_gradient else cout, h, wd), dtype=torch.float32, device=x.device)
    if bias is not None:
        bias = _f32(bias, "bias")
    with torch.cuda.device(x.device):
        _check(_launch(None, 2.0 * b * cout * cin * h * wd, 4.0 * (x.numel() + out.numel() + w.numel()),
                       lambda: lib().sis_conv1x1_f32(_ptr(out), _ptr(x), _ptr(w), _ptr(bias), b, cin, cout, h * wd,
                                                     int(bool(data_gradient)), _stream())), "sis_conv1x1_f32")
    return out


def conv1x1_f32_dgrad_add(grad_output, weight, skip_grad):
    """dL/dx of a 1x1 stride-1 fp32 convolution plus ``skip_grad`` (same shape as the result), one launch."""
    g = _f32(grad_output, "grad_output")
    w = _f32(weight, "weight")
    skip = _f32(skip_grad, "skip_grad")
    b, cout, h, wd = g.shape
    cin = w.shape[1]
    if tuple(skip.shape) != (b, cin, h, wd):
        raise RuntimeError("conv1x1_f32_dgrad_add: skip_grad must have the input's shape")
    out = torch.empty((b, cin, h, wd), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _check(_launch(None, 2.0 * b * cout * cin * h * wd, 4.0 * (g.numel() + 2 * out.numel() + w.numel()),
                       lambda: lib().sis_conv1x1_f32_dgrad_add(_ptr(out), _ptr(g), _ptr(w), _ptr(skip), b, cin, cout, h * wd, _stream())),
               "sis_conv1x1_f32_dgrad_add")
    return out


# ------------------------------------------------------------------------------ bf16 convolutions (matrix cores, NCHW)


_conv_bf16_ok = {}


def conv_bf16_supported(cin, cout, h, w, ksize, stride):
    key = (cin, cout, h, w, ksize, stride)
    hit = _conv_bf16_ok.get(key)
    if hit is None:
        hit = _conv_bf16_ok[key] = bool(lib().sis_conv_bf16_supported(*key))
    return hit


def conv_bf16_pack(weight, h, w, stride=1, adjoint=False):
    """weight [Cout, Cin, k, k] (float32 or bfloat16) -> the kernel's packed LDS image (bf16) for inputs of h x w;
    ``adjoint``: the packing of the data-gradient convolution of a stride-1 layer."""
    require_device(weight, "weight")
    wt = weight.contiguous()
    if wt.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"conv_bf16_pack: weights must be float32 or bfloat16, got {wt.dtype}")
    cout, cin, k, k2 = wt.shape
    n = lib().sis_conv_bf16_packed_elems(cin, cout, h, w, k, stride, int(bool(adjoint)))
    if k != k2 or n < 0:
        raise RuntimeError(f"conv_bf16_pack: unsupported layer {cin}->{cout} k{k}x{k2} s{stride}")
    packed = torch.empty(n, dtype=torch.bfloat16, device=wt.device)
    with torch.cuda.device(wt.device):
        _check(lib().sis_conv_bf16_pack(_ptr(packed), _ptr(wt), _DTYPE_CODE[wt.dtype], cin, cout, h, w, k, stride,
                                        int(bool(adjoint)), _stream()), "sis_conv_bf16_pack")
    return packed


def conv_bf16_pack_both(weight, h, w):
    """Forward and adjoint packings of a stride-1 layer's weight from ONE launch -> (packed, packed_adjoint)."""
    require_device(weight, "weight")
    wt = weight.contiguous()
    cout, cin, k, _ = wt.shape
    n, na = (lib().sis_conv_bf16_packed_elems(cin, cout, h, w, k, 1, a) for a in (0, 1))
    if wt.dtype not in (torch.float32, torch.bfloat16) or n < 0 or na < 0:
        raise RuntimeError(f"conv_bf16_pack_both: unsupported layer {cin}->{cout} k{k} / dtype {wt.dtype}")
    both = torch.empty(n + na, dtype=torch.bfloat16, device=wt.device)
    packed, adjoint = both[:n], both[n:]
    with torch.cuda.device(wt.device):
        _check(lib().sis_conv_bf16_pack_both(_ptr(packed), _ptr(adjoint), _ptr(wt), _DTYPE_CODE[wt.dtype], cin, cout, h, w, k,
                                             _stream()), "sis_conv_bf16_pack_both")
    return packed, adjoint


def conv_bf16(x, packed, cout, ksize, stride=1, bias=None):
    """x [B,Cin,H,W] bf16 (contiguous), packed weights of ``conv_bf16_pack`` -> [B,cout,Ho,Wo] bf16; padding ksize // 2."""
    require_device(x, "input")
    if x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise RuntimeError("conv_bf16: input must be a contiguous bfloat16 tensor")
    b, cin, h, w = x.shape
    pad = ksize // 2
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    y = torch.empty((b, cout, ho, wo), dtype=torch.bfloat16, device=x.device)
    if bias is not None:
        bias = _f32(bias, "bias")
    with torch.cuda.device(x.device):
        _check(_launch(None, 2.0 * b * cout * cin * ksize * ksize * ho * wo, 2.0 * (x.numel() + y.numel() + packed.numel()),
                       lambda: lib().sis_conv_bf16(_ptr(y), _ptr(x), _ptr(packed), _ptr(bias), b, cin, cout, h, w, ksize,
                                                   stride, _stream())), "sis_conv_bf16")
    return y


def conv_bf16_wgrad_supported(batch, cin, cout, h, w):
    return bool(lib().sis_conv_bf16_wgrad_supported(batch, cin, cout, h, w, WORKSPACE_BYTES))


def conv_bf16_wgrad(x, grad_output, out_dtype=torch.float32, for_param=None, defer=False):
    """dL/dw [Cout,Cin,3,3] (float32 or bfloat16) of a stride-1, padding-1 3x3 convolution from its bf16 input and dL/dy.
    ``defer`` (the caller's ``may_complete_late``): the launch waits for ``flush_deferred``, batched with the other layers of its
    shape."""
    require_device(x, "input")
    if x.dtype != torch.bfloat16 or grad_output.dtype != torch.bfloat16 or not x.is_contiguous() or not grad_output.is_contiguous():
        raise RuntimeError("conv_bf16_wgrad: input and grad_output must be contiguous bfloat16 tensors")
    b, cin, h, w = x.shape
    cout = grad_output.shape[1]
    dw = grad_out(for_param, (cout, cin, 3, 3), out_dtype, x.device)
    if defer and _flush_at_end():
        _defer_conv_wgrad(CONV_WGRAD_BF16_3X3, x, grad_output, dw, (b, cin, cout, h, w))
    else:
        _launch_conv_wgrads(CONV_WGRAD_BF16_3X3, (b, cin, cout, h, w), out_dtype, x.device, [(x.data_ptr(), grad_output.data_ptr(), dw.data_ptr())],
                            2.0 * (x.numel() + grad_output.numel()) + 4.0 * dw.numel())
    return dw


def stem_conv_supported(x, weight, stride, padding):
    """The 7x7 stride-2 padding-3 convolution of a 3-channel image to 64 channels (ResNetV2's root) on csrc/stem_conv.hip."""
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and weight.dim() == 4
            and weight.dtype in (torch.float32, torch.bfloat16) and weight.shape[2] == weight.shape[3]
            and bool(lib().sis_stem_conv_supported(x.shape[1], weight.shape[0], weight.shape[2], int(stride), int(padding), x.shape[2], x.shape[3])))


def stem_conv_fwd(x, weight):
    """x [B,3,H,W] (float32 or bfloat16), weight [64,3,7,7] -> y [B,64,Ho,Wo] bfloat16 (bf16 products, fp32 sums)."""
    require_device(x, "input")
    x, w = x.contiguous(), weight.contiguous()
    b, _, h, wd = x.shape
    packed = torch.empty(lib().sis_stem_conv_packed_elems(), dtype=torch.bfloat16, device=x.device)
    y = torch.empty((b, 64, (h - 1) // 2 + 1, (wd - 1) // 2 + 1), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_stem_conv_pack(_ptr(packed), _ptr(w), _DTYPE_CODE[w.dtype], _stream()), "sis_stem_conv_pack")
        _check(_launch(None, 2.0 * y.numel() * 147, 2.0 * y.numel() + x.numel() * x.element_size(),
                       lambda: lib().sis_stem_conv_fwd(_ptr(y), _ptr(x), _DTYPE_CODE[x.dtype], _ptr(packed), b, h, wd, _stream())), "sis_stem_conv_fwd")
    return y


def stem_conv_wgrad(x, grad_y, out_dtype=torch.float32, for_param=None):
    """dL/dw [64,3,7,7] of ``stem_conv_fwd`` from the image and dL/dy (bfloat16)."""
    require_device(x, "input")
    x = x.contiguous()
    gy = grad_y.contiguous()
    if gy.dtype != torch.bfloat16:
        gy = gy.bfloat16()
    b, _, h, wd = x.shape
    dw = grad_out(for_param, (64, 3, 7, 7), out_dtype, x.device)
    ws = _workspace(x.device)
    if lib().sis_stem_conv_wgrad_workspace_bytes(b, h, wd) > ws.numel():
        raise RuntimeError("stem_conv_wgrad: split-K workspace too small (SIS_WORKSPACE_MB)")
    with torch.cuda.device(x.device):
        _check(_launch(None, 2.0 * gy.numel() * 147, 2.0 * gy.numel() + x.numel() * x.element_size(),
                       lambda: lib().sis_stem_conv_wgrad(_ptr(dw), _DTYPE_CODE[out_dtype], _ptr(x), _DTYPE_CODE[x.dtype], _ptr(gy), b, h, wd,
                                                         _ptr(ws), ws.numel(), _stream())), "sis_stem_conv_wgrad")
    return dw


class WeightStdPackBank:
    """Standardised + packed bf16 weights of a list of float32 convolution weights, refreshed by ONE launch
    (``sis_weight_std_pack_multi``).  Output buffers are allocated once: ``w_hat[i]``, ``invstd[i]``, ``packed[i]``,
    ``adjoint[i]`` (None for layers without an adjoint image) keep their addresses, ``refresh()`` rewrites their contents."""

    def __init__(self, weights, strides, eps, standardize=True):
        """``standardize=False``: plain layers (``nn.Conv2d`` of the decoder) -- the launch only rounds to bf16 and packs; ``w_hat``
        / ``invstd`` are lists of None."""
        self.eps = float(eps)
        self.standardize = bool(standardize)
        self.weights = list(weights)
        dev = self.weights[0].device
        self.w_hat, self.invstd, self.packed, self.adjoint = [], [], [], []
        rows, row_begin, filter_begin = [], 0, 0
        for w, stride in zip(self.weights, strides):
            cout, cin, k, _ = w.shape
            mt, kc, mt2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            pe, ae = ctypes.c_int64(), ctypes.c_int64()
            if w.dtype != torch.float32 or not w.is_contiguous() or not lib().sis_weight_std_pack_plan(
                    cin, cout, k, stride, ctypes.byref(mt), ctypes.byref(kc), ctypes.byref(mt2), ctypes.byref(pe), ctypes.byref(ae)):
                raise RuntimeError(f"WeightStdPackBank: no plan for a {cin}->{cout} k{k} s{stride} layer")
            self.w_hat.append(torch.empty(w.shape, dtype=torch.bfloat16, device=dev) if standardize else None)
            self.invstd.append(torch.empty(cout, dtype=torch.float32, device=dev) if standardize else None)
            self.packed.append(torch.empty(pe.value, dtype=torch.bfloat16, device=dev))
            self.adjoint.append(torch.empty(ae.value, dtype=torch.bfloat16, device=dev) if mt2.value else None)
            n_rows = -(-cout // mt.value) * mt.value
            rows.append([w.data_ptr(), self.w_hat[-1].data_ptr() if standardize else 0, self.invstd[-1].data_ptr() if standardize else 0,
                         self.packed[-1].data_ptr(),
                         self.adjoint[-1].data_ptr() if mt2.value else 0, cout, cin, k, mt.value, kc.value, mt2.value, n_rows, row_begin,
                         filter_begin])
            row_begin += n_rows
            filter_begin += cout
        self.total_rows = row_begin
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.source_ptrs = [w.data_ptr() for w in self.weights]

    @staticmethod
    def supported(weight, stride):
        cout, cin, k, k2 = weight.shape
        out = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()]
        return bool(k == k2 and weight.dtype == torch.float32 and weight.is_contiguous()
                    and lib().sis_weight_std_pack_plan(cin, cout, k, stride, *[ctypes.byref(o) for o in out]))

    def current(self):
        """The table still points at the weights (a module moved / re-materialised since would have new storage)."""
        return all(w.data_ptr() == ptr for w, ptr in zip(self.weights, self.source_ptrs))

    def backward(self, grads):
        """grads[i]: dL/dw_hat of layer i or None -> list of dL/dw (float32) or None, one launch for all layers (bf16
        contiguous gradients; anything else goes layer by layer)."""
        n = len(self.weights)
        if any(g is not None and (g.dtype != torch.bfloat16 or not g.is_contiguous()) for g in grads):
            return [None if g is None else weight_std_bwd(g, w, i, self.eps) for g, w, i in zip(grads, self.weights, self.invstd)]
        out = [None if g is None else grad_out(w.data_ptr(), tuple(w.shape), torch.float32, w.device) for g, w in zip(grads, self.weights)]
        g_ptrs = (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in grads])
        o_ptrs = (ctypes.c_void_p * n)(*[None if o is None else o.data_ptr() for o in out])
        couts = (ctypes.c_int * n)(*[w.shape[0] for w in self.weights])
        with torch.cuda.device(self.table.device):
            _check(lib().sis_weight_std_bwd_multi(_ptr(self.table), g_ptrs, o_ptrs, couts, n, _stream()), "sis_weight_std_bwd_multi")
        return out

    def refresh(self):
        with torch.cuda.device(self.table.device):
            _check(lib().sis_weight_std_pack_multi(_ptr(self.table), len(self.weights), self.total_rows, self.eps, _stream()),
                   "sis_weight_std_pack_multi")


class _SwapLast2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _swap_last2(x)

    @staticmethod
    def backward(ctx, grad):
        return _swap_last2(grad.contiguous())


def _swap_last2(x):
    b, r, c = x.shape
    out = torch.empty((b, c, r), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_transpose_batched(_ptr(out), _ptr(x), x.element_size(), b, r, c, _stream()), "sis_transpose_batched")
    return out


def swap_last2(x):
    """Contiguous [B, R, C] -> contiguous [B, C, R] (differentiable): ``x.transpose(-1, -2).contiguous()`` as one tiled kernel."""
    require_device(x, "input")
    if x.dim() != 3 or x.element_size() not in (2, 4) or not x.is_contiguous():
        raise RuntimeError("swap_last2: a contiguous 3-d tensor of 2- or 4-byte elements is required")
    return _SwapLast2.apply(x)


class TransposeBank:
    """Transposed bf16 copies of a list of 2-D bf16 matrices, refreshed by ONE launch (``sis_transpose_bf16_multi``).
    ``out[i]`` ([cols, rows]) keep their addresses; ``refresh()`` rewrites their contents from the sources."""

    def __init__(self, sources):
        self.sources = list(sources)
        dev = self.sources[0].device
        self.out, rows, first = [], [], 0
        for s in self.sources:
            if s.dtype != torch.bfloat16 or s.dim() != 2 or not s.is_contiguous():
                raise RuntimeError("TransposeBank: sources must be contiguous 2-D bfloat16 tensors")
            r, c = s.shape
            self.out.append(torch.empty((c, r), dtype=torch.bfloat16, device=dev))
            rows.append([s.data_ptr(), self.out[-1].data_ptr(), r, c, first])
            first += -(-r // 64) * -(-c // 64)
        self.total_tiles = first
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.source_ptrs = [s.data_ptr() for s in self.sources]

    def current(self, sources):
        return len(sources) == len(self.source_ptrs) and all(s.data_ptr() == p for s, p in zip(sources, self.source_ptrs))

    def refresh(self):
        with torch.cuda.device(self.table.device):
            _check(lib().sis_transpose_bf16_multi(_ptr(self.table), len(self.sources), self.total_tiles, _stream()),
                   "sis_transpose_bf16_multi")


def conv1x1_bf16_wgrad_supported(batch, cin, cout, pixels):
    return bool(lib().sis_conv1x1_bf16_wgrad_supported(batch, cin, cout, pixels, WORKSPACE_BYTES))


def conv1x1_bf16_wgrad(x, grad_output, out_dtype=torch.float32, for_param=None, defer=False):
    """dL/dw [Cout,Cin,1,1] (float32 or bfloat16) of a stride-1 1x1 convolution from its bf16 NCHW input and dL/dy."""
    require_device(x, "input")
    if x.dtype != torch.bfloat16 or grad_output.dtype != torch.bfloat16 or not x.is_contiguous() or not grad_output.is_contiguous():
        raise RuntimeError("conv1x1_bf16_wgrad: input and grad_output must be contiguous bfloat16 tensors")
    b, cin = x.shape[0], x.shape[1]
    cout = grad_output.shape[1]
    pixels = x[0, 0].numel()
    if grad_output.shape[0] != b or grad_output[0, 0].numel() != pixels:
        raise RuntimeError("conv1x1_bf16_wgrad: input and grad_output disagree on batch / plane size")
    dw = grad_out(for_param, (cout, cin, 1, 1), out_dtype, x.device)
    if defer and _flush_at_end():   # (as conv_bf16_wgrad)
        _defer_conv_wgrad(CONV_WGRAD_BF16_1X1, x, grad_output, dw, (b, cin, cout, pixels))
    else:
        _launch_conv_wgrads(CONV_WGRAD_BF16_1X1, (b, cin, cout, pixels), out_dtype, x.device, [(x.data_ptr(), grad_output.data_ptr(), dw.data_ptr())],
                            2.0 * (x.numel() + grad_output.numel()) + 4.0 * dw.numel())
    return dw


# ------------------------------------------------------------------------------ bf16 GEMM with fused epilogues (ViT encoder)

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
TILE_256X96, TILE_256X192, TILE_256X288 = 9, 10, 11   # 256-row tiles of csrc/gemm256_bf16.hip (NT layout, no split-K)


def gemm_tile_256(m, n, k):
    """Tile code of the 256-row GEMM kernel for an [m, n] output contracted over k, or None when the 128-wide tiles of
    csrc/gemm_bf16.hip suit the shape better: the widest of 256 x 288 / 192 / 96 that divides n and still leaves at least
    ~200 tiles for the 256 compute units (8 192 tokens: n = 2304 -> 256 tiles of 256 x 288, 3072 -> 512 of 256 x 192,
    768 -> 256 of 256 x 96)."""
    if k % 64 or k < 128 or n % 4:
        return None
    m_tiles = -(-m // 256)
    for code, width in ((TILE_256X288, 288), (TILE_256X192, 192), (TILE_256X96, 96)):
        if width in _GEMM256_WIDTHS and n % width == 0 and m_tiles * (n // width) >= 200:
            return code
    return None


# Widths of the 256-row tiles the encoder may pick (tools/bench_gemm256.py, 8 192 tokens, against the 128-wide tiles with the
# same epilogues): 256 x 288 wins on the fused projection (46.2 -> 35.0 us), 256 x 192 on fc1 with its GELU + dropout
# epilogue (72.8 -> 66.3 us); 256 x 96 loses on the 768-wide outputs (its 58 B/clk of operand traffic per MFMA cycle is the
# load path's limit, and a single workgroup per CU cannot hide its epilogue: 47 -> 56 us for fc2).
# SIS_GEMM256_TILES=288,192,96 enables all three for measurements.
_GEMM256_WIDTHS = tuple(int(w) for w in os.environ.get("SIS_GEMM256_TILES", "288,192").split(",") if w)
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU_DROP, EPI_BIAS_DROP_RESID, EPI_GELU_BWD, EPI_F32 = range(6)


def _rows2d(t, name):
    if t.dim() != 2 or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16:
        raise RuntimeError(f"gemm_bf16: {name} must be a 2-D bfloat16 tensor with unit column stride, a row stride that is a "
                           "multiple of 8 and a 16-byte aligned base")
    return t


def gemm_bf16(a, b, layout, epilogue=EPI_NONE, bias=None, resid=None, pre=None, seed=None, site=0, drop_p=0.0, splits=1, tile=0, out=None):
    """C = epilogue(op(a) op(b)) on the bf16 matrix cores (csrc/gemm_bf16.hip), fp32 accumulation.
      GEMM_NT  a [m,k], b [n,k]   (forward of a Linear layer: x, weight)
      GEMM_NN  a [m,k], b [k,n]   (data gradient: grad, weight)
      GEMM_TN  a [k,m], b [k,n]   (weight gradient: grad, x; EPI_F32, optionally split over k)
    Row-strided views are taken as they are (row stride % 8 == 0).  Returns C (bf16, or fp32 for EPI_BIAS_DROP_RESID /
    EPI_F32); EPI_BIAS_GELU_DROP returns (dropout(gelu(h)), gelu'(h) * dropout factor) -- the second is the ``pre=`` of EPI_GELU_BWD."""
    require_device(a, "a")
    a, b = _rows2d(a, "a"), _rows2d(b, "b")
    if layout == GEMM_NT:
        (m, k), (n, k2) = a.shape, b.shape
    elif layout == GEMM_NN:
        (m, k), (k2, n) = a.shape, b.shape
    else:
        (k, m), (k2, n) = a.shape, b.shape
    if k != k2:
        raise RuntimeError(f"gemm_bf16: contraction lengths differ ({k} vs {k2})")
    f32_out = epilogue in (EPI_BIAS_DROP_RESID, EPI_F32)
    if out is not None:   # (a weight gradient written into its parameter's arena slice: ``grad_out``)
        if tuple(out.shape) != (m, n) or out.dtype != (torch.float32 if f32_out else torch.bfloat16) or not out.is_contiguous():
            raise RuntimeError("gemm_bf16: out must be a contiguous [m, n] tensor of the result's dtype")
        c = out
    else:
        c = torch.empty((m, n), dtype=torch.float32 if f32_out else torch.bfloat16, device=a.device)
    c2 = torch.empty((m, n), dtype=torch.bfloat16, device=a.device) if epilogue == EPI_BIAS_GELU_DROP else None
    b0, b1, b2, seg = bias, None, None, 0
    if isinstance(bias, (tuple, list)):   # query | key | value: three parameters, one fused projection
        b0, b1, b2 = (_f32(t, "bias") for t in bias)
        seg = b0.numel()
    elif bias is not None:
        b0 = _f32(bias, "bias")
    if resid is not None:
        resid = _f32(resid, "residual")
        if tuple(resid.shape) != (m, n):
            raise RuntimeError("gemm_bf16: the residual must have the output's shape")
    if pre is not None and (pre.dtype != torch.bfloat16 or tuple(pre.shape) != (m, n) or not pre.is_contiguous()):
        raise RuntimeError("gemm_bf16: the pre-activation must be a contiguous bfloat16 tensor of the output's shape")
    ws, ws_bytes = None, 0
    if splits > 1:
        # split-K slabs: one scratch buffer per (device, stream) -- the encoder's weight gradients run on a side stream while
        # the main stream's convolution weight gradients use the per-device buffer
        ws = _stream_workspace(a.device)
        ws_bytes = ws.numel()
    name = f"gemm_bf16<{('NT', 'NN', 'TN')[layout]},{epilogue}>" if tile < TILE_256X96 else f"gemm256<{(96, 192, 288)[tile - TILE_256X96]},{epilogue}>"
    with torch.cuda.device(a.device):
        _check(_launch(name, 2.0 * m * n * k, 2.0 * (m * k + n * k) + c.element_size() * m * n,
                       lambda: lib().sis_gemm_bf16(_ptr(c), _ptr(c2), _ptr(a), _ptr(b), layout, epilogue, m, n, k, a.stride(0),
                                                   b.stride(0), n, _ptr(b0), _ptr(b1), _ptr(b2), seg, _ptr(resid), _ptr(pre), _ptr(seed), int(site),
                                                   float(drop_p), int(splits), _ptr(ws), ws_bytes, int(tile), _stream())),
               "sis_gemm_bf16")
    return (c, c2) if c2 is not None else c


def _stream_workspace(device):
    """Split-K scratch of the current stream (the per-device buffer on the default stream)."""
    stream = torch.cuda.current_stream(device)
    if stream == torch.cuda.default_stream(device):
        return _workspace(device)
    ws = _workspaces.get((device, stream.cuda_stream))
    if ws is None:
        ws = _workspaces[(device, stream.cuda_stream)] = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
    return ws


def gemm_bf16_wgrad_bias(grad, x, splits, tile=0, dw=None):
    """Weight and bias gradient of a Linear layer from dL/dy ``grad`` [tokens, out] and its input ``x`` [tokens, in] (bf16):
    -> (dW [out, in] float32, db [out] float32) in the two launches of the split-K weight-gradient GEMM -- the column sums of
    ``grad`` are computed by extra workgroups of those launches (``sis_gemm_bf16_wgrad_bias``)."""
    require_device(grad, "grad")
    grad, x = _rows2d(grad, "grad"), _rows2d(x, "x")
    (k, m), (k2, n) = grad.shape, x.shape
    if k != k2 or splits < 2 or m % 4:
        raise RuntimeError("gemm_bf16_wgrad_bias: row counts differ, fewer than 2 splits, or an output width that is not a multiple of 4")
    if dw is None:
        dw = torch.empty((m, n), dtype=torch.float32, device=grad.device)
    elif tuple(dw.shape) != (m, n) or dw.dtype != torch.float32 or not dw.is_contiguous():
        raise RuntimeError("gemm_bf16_wgrad_bias: dw must be a contiguous float32 [out, in] tensor")
    db = torch.empty(m, dtype=torch.float32, device=grad.device)
    ws = _stream_workspace(grad.device)
    with torch.cuda.device(grad.device):
        _check(_launch("gemm_bf16<TN,5>", 2.0 * m * n * k, 2.0 * (m * k + n * k) + 4.0 * m * n,
                       lambda: lib().sis_gemm_bf16_wgrad_bias(_ptr(dw), _ptr(db), _ptr(grad), _ptr(x), m, n, k, grad.stride(0), x.stride(0),
                                                              int(splits), _ptr(ws), ws.numel(), int(tile), _stream())),
               "sis_gemm_bf16_wgrad_bias")
    return dw, db


_WGRAD_MULTI_TILE = int(os.environ.get("SIS_WGRAD_MULTI_TILE", "4"))   # 128 x 128 four-wave tile of the batched weight gradients


def gemm_bf16_wgrad_bias_multi(jobs, tile=None):
    """Weight and bias gradients of several Linear layers of ONE shape from one launch (+ one for the column sums):
    ``jobs`` = [(grad [tokens, out] bf16, x [tokens, in] bf16, dw [out, in] float32, db [out] float32), ...] -- or the same as raw
    addresses (grad_ptr, x_ptr, dw_ptr, db_ptr) with ``shape`` = (tokens, out, in, lda, ldb, device) given through ``tile``'s
    sibling ``_wgrad_multi_raw`` (the deferred queue).  Every problem contracts all its tokens per tile: no split-K slabs."""
    g0, x0 = jobs[0][0], jobs[0][1]
    require_device(g0, "grad")
    k, m = g0.shape
    n = x0.shape[1]
    for g, x, dw, db in jobs:
        if (tuple(g.shape) != (k, m) or tuple(x.shape) != (k, n) or g.dtype != torch.bfloat16 or x.dtype != torch.bfloat16
                or g.stride(1) != 1 or x.stride(1) != 1 or g.stride(0) != g0.stride(0) or x.stride(0) != x0.stride(0)
                or tuple(dw.shape) != (m, n) or dw.dtype != torch.float32 or not dw.is_contiguous()
                or tuple(db.shape) != (m,) or db.dtype != torch.float32):
            raise RuntimeError("gemm_bf16_wgrad_bias_multi: every job must have the first job's shapes, strides and dtypes")
    _wgrad_multi_raw([(g.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr()) for g, x, dw, db in jobs],
                     (k, m, n, g0.stride(0), x0.stride(0), g0.device), tile)


def _wgrad_multi_raw(ptrs, shape, tile=None):
    k, m, n, lda, ldb, device = shape
    nj = len(ptrs)
    arr = ctypes.c_void_p * nj
    ws = _stream_workspace(device)
    need = lib().sis_gemm_bf16_wgrad_multi_workspace_bytes(min(nj, 16), m, k)
    if need > ws.numel():
        raise RuntimeError("gemm_bf16_wgrad_bias_multi: split-K workspace too small for the partial column sums")
    with torch.cuda.device(device):
        _check(_launch("gemm_bf16<TN,multi>", 2.0 * m * n * k * nj, (2.0 * (m * k + n * k) + 4.0 * m * n) * nj,
                       lambda: lib().sis_gemm_bf16_wgrad_bias_multi(arr(*[p[2] for p in ptrs]), arr(*[p[3] for p in ptrs]),
                                                                    arr(*[p[0] for p in ptrs]), arr(*[p[1] for p in ptrs]), nj, m, n, k,
                                                                    lda, ldb, _ptr(ws), ws.numel(),
                                                                    _WGRAD_MULTI_TILE if tile is None else int(tile), _stream())),
               "sis_gemm_bf16_wgrad_bias_multi")


def _batched_operand(t, name):
    """[batches, rows, cols] (or [rows, cols], shared by every batch entry) -> (tensor, rows, cols, row stride, batch stride)."""
    if t.dim() == 2:
        t = _rows2d(t, name)
        return t, t.shape[0], t.shape[1], t.stride(0), 0, 1
    if t.dim() != 3 or t.dtype != torch.bfloat16 or t.stride(2) != 1 or t.stride(1) % 8 or t.data_ptr() % 16 or t.stride(0) % 8:
        raise RuntimeError(f"gemm_bf16_batched: {name} must be [batches, rows, cols] bfloat16 with unit column stride and 16-byte aligned rows")
    return t, t.shape[1], t.shape[2], t.stride(1), t.stride(0), t.shape[0]


def gemm_bf16_batched(a, b, layout, epilogue=EPI_NONE, sum_over_batches=False, tile=0):
    """``gemm_bf16`` over a batch of problems in one launch; 2-D operands are shared by all entries.  ``sum_over_batches``:
    one fp32 result = the sum of the entries' products (EPI_F32; 1, 2, 4 or a multiple of 8 entries)."""
    require_device(a, "a")
    a, ar, ac, lda, abs_, na = _batched_operand(a, "a")
    b, br, bc, ldb, bbs, nb = _batched_operand(b, "b")
    batches = max(na, nb)
    if (na not in (1, batches)) or (nb not in (1, batches)):
        raise RuntimeError("gemm_bf16_batched: batch counts differ")
    if layout == GEMM_NT:
        (m, k), (n, k2) = (ar, ac), (br, bc)
    elif layout == GEMM_NN:
        (m, k), (k2, n) = (ar, ac), (br, bc)
    else:
        (k, m), (k2, n) = (ar, ac), (br, bc)
    if k != k2:
        raise RuntimeError(f"gemm_bf16_batched: contraction lengths differ ({k} vs {k2})")
    dtype = torch.float32 if epilogue == EPI_F32 else torch.bfloat16
    c = torch.empty((m, n) if sum_over_batches else (batches, m, n), dtype=dtype, device=a.device)
    ws, ws_bytes = None, 0
    if sum_over_batches and batches > 1:
        ws = _workspace(a.device)
        ws_bytes = ws.numel()
    with torch.cuda.device(a.device):
        _check(_launch(f"gemm_bf16_batched<{('NT', 'NN', 'TN')[layout]}>", 2.0 * batches * m * n * k,
                       2.0 * batches * (m * k + n * k) + c.element_size() * c.numel(),
                       lambda: lib().sis_gemm_bf16_batched(_ptr(c), _ptr(a), _ptr(b), layout, epilogue, m, n, k, lda, ldb, n, batches,
                                                           abs_, bbs, 0 if sum_over_batches else m * n, int(bool(sum_over_batches)),
                                                           _ptr(ws), ws_bytes, int(tile), _stream())), "sis_gemm_bf16_batched")
    return c


def attention_fwd(qkv, heads):
    """qkv bf16 [B, N, 3 * heads * 64] (query | key | value) -> (context bf16 [B, N, heads * 64], lse fp32 [B, heads, N])."""
    require_device(qkv, "qkv")
    if qkv.dtype != torch.bfloat16 or qkv.dim() != 3 or not qkv.is_contiguous() or qkv.shape[2] != 3 * heads * 64:
        raise RuntimeError("attention_fwd: qkv must be a contiguous bfloat16 [B, N, 3 * heads * 64] tensor")
    b, n, _ = qkv.shape
    ctx = torch.empty((b, n, heads * 64), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((b, heads, n), dtype=torch.float32, device=qkv.device)
    flops = 4.0 * b * heads * n * n * 64
    with torch.cuda.device(qkv.device):
        _check(_launch("attn_fwd_kernel", flops, 2.0 * (qkv.numel() + ctx.numel()),
                       lambda: lib().sis_attention_fwd(_ptr(ctx), _ptr(lse), _ptr(qkv), b, n, heads, _stream())), "sis_attention_fwd")
    return ctx, lse


def attention_bwd(d_ctx, qkv, ctx, lse, heads):
    """Gradient of ``attention_fwd`` w.r.t. qkv (bf16, qkv's layout)."""
    if d_ctx.dtype != torch.bfloat16 or not d_ctx.is_contiguous() or d_ctx.shape != ctx.shape:
        raise RuntimeError("attention_bwd: d_ctx must be a contiguous bfloat16 tensor of the context's shape")
    b, n, _ = qkv.shape
    d_qkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    flops = 14.0 * b * heads * n * n * 64   # 7 products (S and dP are recomputed by both kernels)
    with torch.cuda.device(qkv.device):
        _check(_launch("attn_bwd_kernels", flops, 2.0 * (2 * qkv.numel() + 2 * ctx.numel()),
                       lambda: lib().sis_attention_bwd(_ptr(d_qkv), _ptr(delta), _ptr(d_ctx), _ptr(qkv), _ptr(ctx), _ptr(lse), b, n,
                                                       heads, _stream())), "sis_attention_bwd")
    return d_qkv


def ce_dice_supported(logits, labels):
    return (logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16) and logits.dim() >= 3 and 2 <= logits.shape[1] <= 8
            and labels.dtype == torch.int64 and (logits[0, 0].numel() % 4 == 0))


def ce_dice_fwd(logits, labels):
    """logits [B,C,...] (f32 / bf16), labels int64 [B,...] -> (out3 = [0.5 ce + 0.5 dice, ce, dice], stats for the backward)."""
    require_device(logits, "logits")
    logits, labels = logits.contiguous(), labels.contiguous()
    b, c = logits.shape[:2]
    hw = logits[0, 0].numel()
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    stats = torch.empty(1 + 2 * c, dtype=torch.float32, device=logits.device)
    ws = torch.empty(lib().sis_ce_dice_workspace_floats(c), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _check(lib().sis_ce_dice_fwd(_ptr(out), _ptr(stats), _ptr(ws), _ptr(logits), _DTYPE_CODE[logits.dtype], _ptr(labels), b, c, hw,
                                     _stream()), "sis_ce_dice_fwd")
    return out, stats


def ce_dice_bwd(grad_loss, logits, labels, stats):
    logits, labels = logits.contiguous(), labels.contiguous()
    b, c = logits.shape[:2]
    hw = logits[0, 0].numel()
    grad = torch.empty_like(logits)
    if grad_loss is not None:
        grad_loss = _f32(grad_loss, "grad_loss").reshape(1)
    with torch.cuda.device(logits.device):
        _check(lib().sis_ce_dice_bwd(_ptr(grad), _ptr(logits), _DTYPE_CODE[logits.dtype], _ptr(labels), _ptr(stats), _ptr(grad_loss), b, c,
                                     hw, _stream()), "sis_ce_dice_bwd")
    return grad


_drop_seeds = {}


def dropout_seed(device):
    """The device seed word (int64 [1]) every dropout site of the fused ViT kernels reads; initialised from torch's seed."""
    device = torch.device(device)
    t = _drop_seeds.get(device)
    if t is None:
        t = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=device)
        _drop_seeds[device] = t
    return t


def dropout_advance(seed):
    with torch.cuda.device(seed.device):
        _check(lib().sis_dropout_advance(_ptr(seed), _stream()), "sis_dropout_advance")


def dropout_bwd_cast(grad, seed, site, drop_p):
    """bf16(grad * dropout factor): gradient of ``resid + dropout(y)`` w.r.t. y (y dense, row-major, grad fp32)."""
    grad = _f32(grad, "grad")
    out = torch.empty(grad.shape, dtype=torch.bfloat16, device=grad.device)
    with torch.cuda.device(grad.device):
        _check(lib().sis_dropout_bwd_cast(_ptr(out), _ptr(grad), grad.numel(), _ptr(seed), int(site), float(drop_p), _stream()),
               "sis_dropout_bwd_cast")
    return out


# ------------------------------------------------------------------------------ layer norm


def layer_norm_supported(x, n):
    return x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and n in (256, 512, 768, 1024) and x.shape[-1] == n


def layer_norm_fwd(x, gamma, beta, eps, out_dtype=None):
    """x [..., n] (f32 / bf16) -> (y in ``out_dtype``, mean [rows], rstd [rows])."""
    require_device(x, "input")
    x = x.contiguous()
    out_dtype = out_dtype or x.dtype
    n = x.shape[-1]
    rows = x.numel() // n
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with torch.cuda.device(x.device):
        _check(lib().sis_layer_norm_fwd(_ptr(y), _ptr(mean), _ptr(rstd), _ptr(x), _ptr(_f32(gamma, "weight")),
                                        _ptr(_f32(beta, "bias")), _DTYPE_CODE[x.dtype], _DTYPE_CODE[out_dtype], rows, n,
                                        float(eps), _stream()), "sis_layer_norm_fwd")
    return y, mean, rstd


def layer_norm_bwd_fused(grad_y, x, mean, rstd, gamma, residual_grad=None, cast_seed=None, cast_site=None, cast_p=0.0, defer=False):
    """LayerNorm backward of a pre-norm residual block: dx = residual_grad + LN'(grad_y); with ``cast_site`` also returns
    bf16(dx * dropout factor of that site) -> (dx, dgamma, dbeta, cast or None).  ``defer`` (the caller's
    ``may_complete_late`` for the two parameters): the reduction to dgamma / dbeta joins the deferred queue (``flush_deferred``)."""
    x = x.contiguous()
    g = grad_y.contiguous()
    n = x.shape[-1]
    rows = x.numel() // n
    dx = torch.empty_like(x)
    dgamma = torch.empty(n, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    cast = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if cast_site is not None else None
    if residual_grad is not None:
        residual_grad = _f32(residual_grad, "residual_grad")
    ws = torch.empty(lib().sis_layer_norm_workspace_floats(n), dtype=torch.float32, device=x.device)
    if defer and _flush_at_end():   # d(gamma) / d(beta) by the batched reduction at the end of the backward (flush_deferred)
        with torch.cuda.device(x.device):
            _check(lib().sis_layer_norm_bwd_fused_partial(_ptr(dx), _ptr(ws), _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                                          _DTYPE_CODE[x.dtype], _DTYPE_CODE[g.dtype], rows, n, _ptr(residual_grad),
                                                          _ptr(cast), _ptr(cast_seed), int(cast_site or 0), float(cast_p), _stream()),
                   "sis_layer_norm_bwd_fused_partial")
        _deferred["ln"].append((dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), int(lib().sis_layer_norm_bwd_parts(rows)), n, x.device,
                                _hold(dgamma, dbeta, ws)))
        return dx, dgamma, dbeta, cast
    with torch.cuda.device(x.device):
        _check(lib().sis_layer_norm_bwd_fused(_ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd),
                                              _ptr(gamma), _DTYPE_CODE[x.dtype], _DTYPE_CODE[g.dtype], rows, n, _ptr(residual_grad),
                                              _ptr(cast), _ptr(cast_seed), int(cast_site or 0), float(cast_p), _stream()),
               "sis_layer_norm_bwd_fused")
    return dx, dgamma, dbeta, cast


def layer_norm_bwd(grad_y, x, mean, rstd, gamma):
    x = x.contiguous()
    g = grad_y.contiguous()
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    n = x.shape[-1]
    rows = x.numel() // n
    dx = torch.empty_like(x)
    dgamma = torch.empty(n, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = torch.empty(lib().sis_layer_norm_workspace_floats(n), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_layer_norm_bwd(_ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd),
                                        _ptr(gamma), _DTYPE_CODE[x.dtype], _DTYPE_CODE[g.dtype], rows, n, _stream()),
               "sis_layer_norm_bwd")
    return dx, dgamma, dbeta


def column_sum(x):
    """x [rows, n] (f32 / f16 / bf16, n % 4 == 0) -> float32 [n] column sums (bias gradient of a Linear layer)."""
    require_device(x, "input")
    x = x.contiguous()
    rows, n = x.shape
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib().sis_column_sum_workspace_floats(n), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_column_sum(_ptr(out), _ptr(ws), _ptr(x), _DTYPE_CODE[x.dtype], rows, n, _stream()), "sis_column_sum")
    return out


# ------------------------------------------------------------------------------ group norm (+ ReLU)


_GROUP_COUNTERS = {}  # (device, stream) -> int32 zeros: completion counters of the norm kernels (each launch leaves them zero)
_GROUP_COUNTER_ROWS = 1 << 16   # sized up front: a captured hipGraph holds the buffer's address, so it is never reallocated
_GN_FUSED_FINISH = os.environ.get("SIS_GN_FUSED_FINISH", "1") != "0"  # 0: the per-group merges as launches of their own


def _group_counters(device, n):
    """Completion counters of the in-launch hand-over (csrc/sis_xwg.h), one buffer per (device, stream) like the split-K
    scratch: launches on one stream are ordered, and every launch leaves its counters at zero, so concurrent streams must not
    share them.  The buffer has a fixed size -- pointers baked into a captured graph stay valid -- and a launch
    that would need more rows falls back to the merge-as-its-own-launch form (returns None)."""
    if not _GN_FUSED_FINISH or n > _GROUP_COUNTER_ROWS:
        return None
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _GROUP_COUNTERS.get(key)
    if buf is None:
        buf = _GROUP_COUNTERS[key] = torch.zeros(_GROUP_COUNTER_ROWS, dtype=torch.int32, device=device)
    return buf


def prepare_capture(device):
    """Called on the stream a hipGraph capture is about to run on, BEFORE the capture opens: creates (and zeroes, as ordinary
    eager stream work) the per-stream state that captured launches will hold pointers to -- the completion counters and the
    split-K scratch -- so that neither lives in the graph's private pool with its zero-fill as a captured node only (ADVICE r4:
    a failed capture would leave a cached, never-zeroed counter buffer behind for the next capture on that stream).
    Returns a snapshot for ``rollback_capture``."""
    _group_counters(device, 1)
    _stream_workspace(device)
    return (set(_GROUP_COUNTERS), set(_workspaces))


def rollback_capture(snapshot):
    """After a FAILED capture: forget per-stream buffers that were first created while the capture was open."""
    counters, workspaces = snapshot
    for key in [k for k in _GROUP_COUNTERS if k not in counters]:
        del _GROUP_COUNTERS[key]
    for key in [k for k in _workspaces if k not in workspaces]:
        del _workspaces[key]


def group_counters_are_zero():
    """Debug check (tests): every completion-counter buffer is back at zero, i.e. no launch left a hand-over half done."""
    return all(int(buf.abs().max().item()) == 0 for buf in _GROUP_COUNTERS.values())


def group_norm_fwd(x, gamma, beta, groups, eps, relu, out_dtype=None, residual=None, low_precision_copy=False, want_gate=False):
    """x [B,C,...] (f32 / f16 / bf16) -> (y in ``out_dtype`` (default: x's), mean [B*groups], rstd [B*groups]).
    ``residual`` (float32, x's shape) is added before the ReLU; the output is then float32.
    ``low_precision_copy`` (16-bit x, float32 y): also returns y rounded to x's dtype, written in the same pass
    -> (y, mean, rstd, y_lp).  ``want_gate`` (with relu): one more result, the ReLU gate [y > 0] as one bit per element (uint8
    tensor) that ``group_norm_bwd(..., gate=...)`` reads instead of the saved output."""
    require_device(x, "input")
    x = x.contiguous()
    if residual is not None:
        out_dtype = torch.float32
        residual = _f32(residual, "residual")
        if residual.shape != x.shape:
            raise RuntimeError("residual must have the input's shape")
    out_dtype = out_dtype or x.dtype
    if low_precision_copy and not (out_dtype == torch.float32 and x.dtype in (torch.float16, torch.bfloat16)):
        raise RuntimeError("low_precision_copy needs a float32 output of a 16-bit input")
    b, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    y_lp = torch.empty_like(x) if low_precision_copy else None
    mean = torch.empty(b * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = torch.empty(lib().sis_group_norm_workspace_floats(b, c, hw), dtype=torch.float32, device=x.device)
    gate = torch.empty(lib().sis_group_norm_gate_bytes(b, c, hw), dtype=torch.uint8, device=x.device) if (want_gate and relu) else None
    with torch.cuda.device(x.device):
        _check(lib().sis_group_norm_fwd(_ptr(y), _ptr(y_lp), _ptr(mean), _ptr(rstd), _ptr(ws), _ptr(x), _ptr(residual),
                                        _ptr(_f32(gamma, "weight")), _ptr(_f32(beta, "bias")), _DTYPE_CODE[x.dtype],
                                        _DTYPE_CODE[out_dtype], b, c, hw, groups, float(eps), int(bool(relu)),
                                        _ptr(_group_counters(x.device, b * groups)), _ptr(gate), _stream()),
               "sis_group_norm_fwd")
    out = (y, mean, rstd, y_lp) if low_precision_copy else (y, mean, rstd)
    return out + (gate,) if want_gate else out


def group_norm_bwd(grad_y, x, mean, rstd, gamma, beta, groups, relu, y_mask=None, want_residual_grad=False, grad_y_lp=None, gate=None):
    """-> (dx, dgamma, dbeta[, dresidual]).  ``y_mask``: the saved float32 output when a residual was added (its sign is
    the ReLU mask); ``want_residual_grad`` also returns the gradient of the residual branch; ``grad_y_lp`` (x's 16-bit
    dtype): the gradient that came back through the low-precision copy of the output, added to ``grad_y`` (float32) on load."""
    x = x.contiguous()
    g = grad_y.contiguous()
    if g.dtype != x.dtype and g.dtype != torch.float32:
        g = g.to(x.dtype)
    if grad_y_lp is not None:
        if g.dtype != torch.float32 or grad_y_lp.dtype != x.dtype or x.dtype == torch.float32:
            raise RuntimeError("grad_y_lp needs a float32 grad_y and the 16-bit dtype of x")
        grad_y_lp = grad_y_lp.contiguous()
    b, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    dx = torch.empty_like(x)
    dres = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_residual_grad else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = torch.empty(lib().sis_group_norm_workspace_floats(b, c, hw), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_group_norm_bwd(_ptr(dx), _ptr(dres), _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(g), _ptr(grad_y_lp), _ptr(x),
                                        _ptr(y_mask), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _DTYPE_CODE[x.dtype],
                                        _DTYPE_CODE[g.dtype], b, c, hw, groups, int(bool(relu)),
                                        _ptr(_group_counters(x.device, b * groups)), _ptr(gate), _stream()), "sis_group_norm_bwd")
    return (dx, dgamma, dbeta, dres) if want_residual_grad else (dx, dgamma, dbeta)


def batch_norm_train_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, relu, out_dtype=None):
    """Training-mode batch norm (+ ReLU) on f32 / f16 / bf16 tensors -> (y, mean [C], rstd [C])."""
    require_device(x, "input")
    x = x.contiguous()
    out_dtype = out_dtype or x.dtype
    b, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = torch.empty(lib().sis_group_norm_workspace_floats(b, c, hw), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_batch_norm_fwd(_ptr(y), _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var), _ptr(ws), _ptr(x),
                                        _ptr(_f32(gamma, "weight")), _ptr(_f32(beta, "bias")), _DTYPE_CODE[x.dtype],
                                        _DTYPE_CODE[out_dtype], b, c, hw, float(eps), float(momentum), int(bool(relu)),
                                        _ptr(_group_counters(x.device, c)), _stream()), "sis_batch_norm_fwd")
    return y, mean, rstd


def batch_norm_train_bwd(grad_y, x, mean, rstd, gamma, beta, relu):
    x = x.contiguous()
    g = grad_y.contiguous()
    if g.dtype != x.dtype and g.dtype != torch.float32:
        g = g.to(x.dtype)
    b, c = x.shape[0], x.shape[1]
    hw = x[0, 0].numel()
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    ws = torch.empty(lib().sis_group_norm_workspace_floats(b, c, hw), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_batch_norm_bwd(_ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd),
                                        _ptr(gamma), _ptr(beta), _DTYPE_CODE[x.dtype], _DTYPE_CODE[g.dtype], b, c, hw,
                                        int(bool(relu)), _ptr(_group_counters(x.device, c)), _stream()), "sis_batch_norm_bwd")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------ weight standardisation


def weight_std_fwd(weight, eps, out_dtype=torch.float32):
    """weight [Cout, ...] float32 -> (w_hat in ``out_dtype``, invstd [Cout]) standardised per output channel."""
    w = _f32(weight, "weight")
    rows, n = w.shape[0], w[0].numel()
    w_hat = torch.empty(w.shape, dtype=out_dtype, device=w.device)
    invstd = torch.empty(rows, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(lib().sis_weight_std_fwd(_ptr(w_hat), _ptr(invstd), _ptr(w), _DTYPE_CODE[out_dtype], rows, n, float(eps),
                                        _stream()), "sis_weight_std_fwd")
    return w_hat, invstd


def weight_std_bwd(grad_w_hat, weight, invstd, eps):
    w = _f32(weight, "weight")
    g = grad_w_hat.contiguous()
    rows, n = w.shape[0], w[0].numel()
    dw = torch.empty_like(w)
    with torch.cuda.device(w.device):
        _check(lib().sis_weight_std_bwd(_ptr(dw), _ptr(g), _ptr(w), _ptr(invstd), _DTYPE_CODE[g.dtype], rows, n, float(eps),
                                        _stream()), "sis_weight_std_bwd")
    return dw


# ------------------------------------------------------------------------------ bilinear upsampling (align_corners)


def upsample_bilinear(x, out_h, out_w, grad_output=None):
    """Forward: x [B,C,H,W] -> [B,C,out_h,out_w].  With ``grad_output`` [B,C,out_h,out_w]: the gradient w.r.t. an input
    of x's shape (x is only used for its shape / dtype)."""
    require_device(x, "input")
    if x.dtype not in _DTYPE_CODE or x.dtype == torch.float64:
        raise RuntimeError(f"upsample_bilinear: dtype {x.dtype} not supported")
    b, c, h, w = x.shape
    if grad_output is None:
        src, out, backward = x.contiguous(), torch.empty((b, c, out_h, out_w), dtype=x.dtype, device=x.device), 0
    else:
        src, out, backward = grad_output.contiguous(), torch.empty((b, c, h, w), dtype=x.dtype, device=x.device), 1
    with torch.cuda.device(x.device):
        _check(lib().sis_upsample_bilinear(_ptr(out), _ptr(src), _DTYPE_CODE[x.dtype], b * c, h, w, out_h, out_w, backward,
                                           _stream()), "sis_upsample_bilinear")
    return out


def upsample2x_into(out, x):
    """Bilinear x2 upsampling (align_corners=True) of x [B,C,H,W] into the leading C channels of ``out`` [B,C+S,2H,2W]
    (contiguous; the remaining S channels are left alone)."""
    require_device(x, "input")
    b, c, h, w = x.shape
    if out.shape[0] != b or out.shape[1] < c or out.shape[2:] != (2 * h, 2 * w) or out.dtype != x.dtype or not out.is_contiguous():
        raise RuntimeError("upsample2x_into: out must be a contiguous [B, >= C, 2H, 2W] tensor of the input's dtype")
    with torch.cuda.device(x.device):
        _check(lib().sis_upsample_bilinear_strided(_ptr(out), _ptr(x.contiguous()), _DTYPE_CODE[x.dtype], b, c, h, w, 2 * h, 2 * w,
                                                   out.stride(0), 0, _stream()), "sis_upsample_bilinear_strided")
    return out


def upsample2x_grad_from(grad_wide, channels):
    """Gradient of ``upsample2x_into`` w.r.t. x from the gradient of the WIDE tensor [B,C+S,2H,2W] (contiguous; 16-byte aligned
    images): reads its leading ``channels`` channels in place -> [B,channels,H,W]."""
    require_device(grad_wide, "grad")
    b, ct, oh, ow = grad_wide.shape
    if not grad_wide.is_contiguous() or oh % 2 or ow % 2 or channels > ct:
        raise RuntimeError("upsample2x_grad_from: a contiguous [B, >= C, 2H, 2W] gradient is required")
    gx = torch.empty((b, channels, oh // 2, ow // 2), dtype=grad_wide.dtype, device=grad_wide.device)
    with torch.cuda.device(grad_wide.device):
        _check(lib().sis_upsample_bilinear_strided(_ptr(gx), _ptr(grad_wide), _DTYPE_CODE[grad_wide.dtype], b, channels, oh // 2, ow // 2,
                                                   oh, ow, grad_wide.stride(0), 1, _stream()), "sis_upsample_bilinear_strided")
    return gx


def conv1x1_wgrad_f32_supported(grad_output, input):
    return bool(grad_output.is_cuda and input.is_cuda and grad_output.dtype == torch.float32 and input.dtype == torch.float32
                and grad_output.dim() == 4 and input.dim() == 4 and grad_output.is_contiguous() and input.is_contiguous()
                and lib().sis_conv1x1_wgrad_f32_supported(input.shape[0], input.shape[1], grad_output.shape[1],
                                                         input.shape[2] * input.shape[3]))


def conv1x1_wgrad_f32(grad_output, input, for_param=None, defer=False):
    """dW [Cout, Cin, 1, 1] of a 1x1 stride-1 convolution from dL/dy [B,Cout,H,W] and x [B,Cin,H,W] (fp32, NCHW).  ``defer``: as
    ``conv_bf16_wgrad``."""
    require_device(input, "input")
    b, cin, h, w = input.shape
    cout = grad_output.shape[1]
    dw = grad_out(for_param, (cout, cin, 1, 1), torch.float32, input.device)
    if (defer and _flush_at_end() and grad_output.dtype == torch.float32 and input.dtype == torch.float32
            and grad_output.is_contiguous() and input.is_contiguous() and grad_output.data_ptr() % 16 == 0 and input.data_ptr() % 16 == 0):
        _defer_conv_wgrad(CONV_WGRAD_F32_1X1, input, grad_output, dw, (b, cin, cout, h * w))
        return dw
    # a scratch of exactly the planned slabs (none for a single K slice), not the shared workspace
    ws_bytes = int(lib().sis_conv1x1_wgrad_f32_workspace(b, cin, cout, h * w))
    ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=input.device)
    _launch_conv_wgrads(CONV_WGRAD_F32_1X1, (b, cin, cout, h * w), dw.dtype, input.device,
                        [(input.data_ptr(), grad_output.data_ptr(), dw.data_ptr())],
                        4.0 * (grad_output.numel() + input.numel() + dw.numel()), workspace=(ws if ws_bytes else None, ws_bytes))
    return dw


# ------------------------------------------------------------------------------ max pooling


def max_pool2d(x, kernel, stride, padding):
    """x [B,C,H,W] -> (out [B,C,Ho,Wo], argmax uint8 [B,C,Ho,Wo]); floor mode, dilation 1 (ATen's output size rule)."""
    require_device(x, "input")
    if x.dtype not in _DTYPE_CODE or x.dtype == torch.float64:
        raise RuntimeError(f"max_pool2d: dtype {x.dtype} not supported")
    b, c, h, w = x.shape
    oh, ow = (h + 2 * padding - kernel) // stride + 1, (w + 2 * padding - kernel) // stride + 1
    x = x.contiguous()
    out = torch.empty((b, c, oh, ow), dtype=x.dtype, device=x.device)
    arg = torch.empty((b, c, oh, ow), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_max_pool2d(_ptr(out), _ptr(arg), _ptr(x), _DTYPE_CODE[x.dtype], b * c, h, w, oh, ow, kernel, stride,
                                    padding, 0, _stream()), "sis_max_pool2d")
    return out, arg


def max_pool2d_backward(grad_output, argmax, in_h, in_w, kernel, stride, padding):
    require_device(grad_output, "grad_output")
    b, c, oh, ow = grad_output.shape
    g = grad_output.contiguous()
    dx = torch.empty((b, c, in_h, in_w), dtype=g.dtype, device=g.device)
    with torch.cuda.device(g.device):
        _check(lib().sis_max_pool2d(_ptr(dx), _ptr(argmax), _ptr(g), _DTYPE_CODE[g.dtype], b * c, in_h, in_w, oh, ow, kernel,
                                    stride, padding, 1, _stream()), "sis_max_pool2d")
    return dx


# ------------------------------------------------------------------------------ patch-wise page inference


def _grid(xs, ys, device):
    xs = torch.as_tensor(xs, dtype=torch.int32).to(device).contiguous()
    ys = torch.as_tensor(ys, dtype=torch.int32).to(device).contiguous()
    return xs, ys


def crop_patches_u8(image, xs, ys, patch):
    """uint8 [H,W,C] page on the device -> float32 [len(ys)*len(xs), C, patch, patch] in [-1,1] (zero padding outside
    the page, ToTensor + Normalize(0.5, 0.5)); patch n = yi * len(xs) + xi."""
    require_device(image, "image")
    if image.dtype != torch.uint8 or image.dim() != 3:
        raise RuntimeError("image must be a uint8 [H, W, C] tensor")
    image = image.contiguous()
    h, w, c = image.shape
    xs, ys = _grid(xs, ys, image.device)
    out = torch.empty((ys.numel() * xs.numel(), c, patch, patch), dtype=torch.float32, device=image.device)
    with torch.cuda.device(image.device):
        _check(lib().sis_crop_patches_u8(_ptr(out), _ptr(image), _ptr(xs), _ptr(ys), xs.numel(), ys.numel(), h, w, c,
                                         patch, _stream()), "sis_crop_patches_u8")
    return out


def assemble_max(pred, xs, ys, height, width, with_labels=False):
    """[N,C,P,P] patch predictions -> [C,height,width] maximum over the covering patches (+ uint8 label map)."""
    pred = _f32(pred, "predictions")
    n, c, p, p2 = pred.shape
    xs, ys = _grid(xs, ys, pred.device)
    if p != p2 or n != xs.numel() * ys.numel():
        raise RuntimeError(f"predictions {tuple(pred.shape)} do not match a {ys.numel()} x {xs.numel()} patch grid")
    out = torch.empty((c, height, width), dtype=torch.float32, device=pred.device)
    labels = torch.empty((height, width), dtype=torch.uint8, device=pred.device) if with_labels else None
    with torch.cuda.device(pred.device):
        _check(lib().sis_assemble_max(_ptr(out), _ptr(labels), _ptr(pred), _ptr(xs), _ptr(ys), xs.numel(), ys.numel(), c,
                                      height, width, p, _stream()), "sis_assemble_max")
    return (out, labels) if with_labels else out


def assemble_vote(pred, xs, ys, height, width, with_labels=False):
    """[N,C,P,P] patch predictions -> [C,height,width] confidences summed over the covering patches (row-major patch order) and
    divided by their sum over the classes, 0 where that sum is 0 (+ uint8 label map, first maximal class)."""
    pred = _f32(pred, "predictions")
    n, c, p, p2 = pred.shape
    xs, ys = _grid(xs, ys, pred.device)
    if p != p2 or n != xs.numel() * ys.numel():
        raise RuntimeError(f"predictions {tuple(pred.shape)} do not match a {ys.numel()} x {xs.numel()} patch grid")
    out = torch.empty((c, height, width), dtype=torch.float32, device=pred.device)
    labels = torch.empty((height, width), dtype=torch.uint8, device=pred.device) if with_labels else None
    with torch.cuda.device(pred.device):
        _check(lib().sis_assemble_vote(_ptr(out), _ptr(labels), _ptr(pred), _ptr(xs), _ptr(ys), xs.numel(), ys.numel(), c,
                                       height, width, p, _stream()), "sis_assemble_vote")
    return (out, labels) if with_labels else out


def confusion_matrix(prediction, ground_truth, num_classes, out=None):
    """int64 [C,C] on the device, rows ground truth, columns prediction.  ``prediction``: float32 confidences [C,H,W] (first
    maximal class) or a uint8 label map [H,W]; ``ground_truth``: uint8 [H,W].  ``out``: a matrix to accumulate into (a run over
    many pages then crosses to the host once); a fresh zeroed one otherwise."""
    require_device(prediction, "prediction")
    require_device(ground_truth, "ground_truth")
    if ground_truth.dtype != torch.uint8 or ground_truth.dim() != 2:
        raise RuntimeError("ground_truth must be a uint8 [H, W] tensor")
    gt = ground_truth.contiguous()
    if prediction.dim() == 3:
        conf, labels = _f32(prediction, "prediction"), None
        if conf.shape[0] != num_classes:
            raise RuntimeError(f"prediction has {conf.shape[0]} classes, expected {num_classes}")
    elif prediction.dim() == 2 and prediction.dtype == torch.uint8:
        conf, labels = None, prediction.contiguous()
    else:
        raise RuntimeError("prediction must be float32 [C, H, W] confidences or a uint8 [H, W] label map")
    if tuple(prediction.shape[-2:]) != tuple(gt.shape):
        raise RuntimeError("Shapes of prediction and ground truth do not match")
    if out is None:
        out = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=gt.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (num_classes, num_classes) or not out.is_contiguous() or out.device != gt.device:
        raise RuntimeError("out must be a contiguous int64 [C, C] tensor on the device of the inputs")
    with torch.cuda.device(gt.device):
        _check(lib().sis_confusion_matrix(_ptr(out), _ptr(conf), _ptr(labels), _ptr(gt), gt.numel(), int(num_classes), _stream()),
               "sis_confusion_matrix")
    return out


def color_to_class(image, colors, ids, background_id=0):
    """uint8 [H,W,3] image on the device -> uint8 [H,W] class ids: ``ids[k]`` where the pixel equals ``colors[k]`` (r, g, b; the
    last match wins), ``background_id`` elsewhere."""
    require_device(image, "image")
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise RuntimeError("image must be a uint8 [H, W, 3] tensor")
    image = image.contiguous()
    n = len(ids)
    flat = [int(v) for color in colors for v in color]
    if len(flat) != 3 * n or any(not 0 <= v <= 255 for v in flat) or any(not 0 <= int(i) <= 255 for i in ids):
        raise RuntimeError("colors must be (r, g, b) byte triples, one per id")
    out = torch.empty(image.shape[:2], dtype=torch.uint8, device=image.device)
    c_colors, c_ids = (ctypes.c_uint8 * max(3 * n, 1))(*flat), (ctypes.c_uint8 * max(n, 1))(*[int(i) for i in ids])
    with torch.cuda.device(image.device):
        _check(lib().sis_color_to_class(_ptr(out), _ptr(image), out.numel(), int(background_id), c_colors, c_ids, n, _stream()),
               "sis_color_to_class")
    return out


def remove_small_contours(pred, min_confidence, min_contour_area, background_class_id=0):
    """BaseSegmenter.postprocess on the device: pred [B,C,P,P] float32 -> pred below ``min_confidence`` zeroed, then every
    region (outermost contour, holes filled) of a non-background plane with a contour area below ``min_contour_area`` zeroed
    (DESIGN.md §10).  One read of ``pred``; the scratch is a torch allocation, so the call can be captured in a graph."""
    pred = _f32(pred, "predictions")
    if pred.dim() != 4 or pred.shape[2] != pred.shape[3]:
        raise RuntimeError(f"predictions must be [B, C, P, P], got {tuple(pred.shape)}")
    b, c, p, _ = pred.shape
    out = torch.empty_like(pred)
    nbytes = int(lib().sis_contour_workspace_bytes(b * c, p))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=pred.device)
    with torch.cuda.device(pred.device):
        _check(_launch("contour_filter", 0.0, 8.0 * pred.numel(),
                       lambda: lib().sis_remove_small_contours(_ptr(out), _ptr(pred), _ptr(ws), ws.numel() * 4, b, c, p,
                                                               float(min_confidence), int(min_contour_area),
                                                               int(background_class_id), _stream())),
               "sis_remove_small_contours")
    return out


def cluster_segment(cluster_maps, lut, determination_sources, fine_sources, fine_class, class_ids, colours, size,
                    only_keep_overlapping, min_class_contour_area):
    """The cluster-based labeller on the device: ``cluster_maps`` int64 [B, r_k, r_k] tensors (FactorCatalog.predict),
    ``lut`` uint8 [len(cluster_maps), 256] on the device (bit c: the cluster belongs to non-background class c),
    ``determination_sources`` / ``fine_sources`` one bitmask over ``cluster_maps`` per key of the step, ``class_ids`` /
    ``colours`` with the background first.  Returns (class_map uint8 [B,S,S], colour uint8 [B,S,S,3], drop uint8 [B]) on the
    device; nothing is read back and the scratch is a torch allocation, so the call can be captured in a graph."""
    maps = []
    for m in cluster_maps:
        require_device(m, "cluster maps")
        if m.dtype != torch.int64 or m.dim() != 3 or m.shape[1] != m.shape[2] or m.shape[0] != cluster_maps[0].shape[0]:
            raise RuntimeError(f"cluster maps must be int64 [B, r, r], got {m.dtype} {tuple(m.shape)}")
        if m.shape[1] > size:
            raise ValueError(f"a cluster map of edge {m.shape[1]} is larger than the image size {size}")
        maps.append(m.contiguous())
    device, b, classes = maps[0].device, maps[0].shape[0], len(class_ids) - 1
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (len(maps), 256) or lut.device != device or not lut.is_contiguous():
        raise RuntimeError("lut must be a contiguous uint8 [keys, 256] tensor on the cluster maps' device")
    if len(colours) != classes + 1 or any(len(c) != 3 for c in colours):
        raise RuntimeError("colours must be one (r, g, b) triple per class id")
    class_map = torch.empty((b, size, size), dtype=torch.uint8, device=device)
    colour = torch.empty((b, size, size, 3), dtype=torch.uint8, device=device)
    drop = torch.empty((b,), dtype=torch.uint8, device=device)
    nd, nf = len(determination_sources), len(fine_sources)
    nbytes = int(lib().sis_cluster_segment_workspace_bytes(b, size, nd, nf, classes))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)   # the caching allocator aligns to 512 bytes
    c_maps = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    c_res = (ctypes.c_int * len(maps))(*[m.shape[1] for m in maps])
    c_det = (ctypes.c_uint8 * max(nd, 1))(*[int(s) for s in determination_sources])
    c_fine = (ctypes.c_uint8 * max(nf, 1))(*[int(s) for s in fine_sources])
    c_ids = (ctypes.c_uint8 * (classes + 1))(*[int(i) for i in class_ids])
    c_col = (ctypes.c_uint8 * (3 * (classes + 1)))(*[int(v) for c in colours for v in c])
    with torch.cuda.device(device):
        _check(_launch("cluster_segment", 0.0, 4.0 * class_map.numel(),
                       lambda: lib().sis_cluster_segment(_ptr(class_map), _ptr(colour), _ptr(drop), c_maps, c_res, len(maps),
                                                         _ptr(lut), c_det, nd, c_fine, nf, classes, int(fine_class), c_ids,
                                                         c_col, b, int(size), int(bool(only_keep_overlapping)),
                                                         int(min_class_contour_area), _ptr(ws), ws.numel(), _stream())),
               "sis_cluster_segment")
    return class_map, colour, drop


# ------------------------------------------------------------------------------ fused batch norm


def bn_supported(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (x.shape[2] * x.shape[3]) % 4 == 0 and x.is_contiguous()


def bn_stats(x, running_mean, running_var, eps, momentum):
    b, c, h, w = x.shape
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib().sis_bn_workspace_floats(b, c, h * w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_bn_stats(_ptr(mean), _ptr(invstd), _ptr(running_mean), _ptr(running_var), _ptr(x), _ptr(ws), b, c,
                                  h * w, float(eps), float(momentum), _stream()), "sis_bn_stats")
    return mean, invstd


def bn_fused_supported(x):
    b, c, h, w = x.shape
    return bool(lib().sis_bn_fused_supported(b, c, h * w))


def bn_fused_fwd(x, residual, gamma, beta, running_mean, running_var, eps, momentum, relu, want_mask=False):
    """``bn_stats`` + ``bn_act_fwd`` in one launch (a channel's batch * H * W values fit one workgroup: ``bn_fused_supported``)
    -> (y, mean, invstd, mask or None)."""
    b, c, h, w = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    mask = torch.empty(lib().sis_bn_mask_words(b, c, h * w), dtype=torch.int64, device=x.device) if (want_mask and relu) else None
    with torch.cuda.device(x.device):
        # (kernel name reported by the library: bn_fused_fwd_kernel, or bn_wide_fwd_kernel for channels of 16 385 ... 65 536 values)
        _check(_launch(None, 0.0, 4.0 * (2 + (residual is not None)) * x.numel(), lambda: lib().sis_bn_fused_fwd(
            _ptr(y), _ptr(mean), _ptr(invstd), _ptr(running_mean), _ptr(running_var), _ptr(x), _ptr(residual),
            _ptr(gamma), _ptr(beta), b, c, h * w, float(eps), float(momentum), int(bool(relu)), _ptr(mask),
            _stream())), "sis_bn_fused_fwd")
    return y, mean, invstd, mask


def bn_act_fwd(x, residual, mean, invstd, gamma, beta, relu, want_mask=False):
    """y = [relu](bn(x) [+ residual]); ``want_mask`` (with relu): also the 1-bit-per-element sign mask the backward can read
    instead of y -> (y, mask)."""
    b, c, h, w = x.shape
    y = torch.empty_like(x)
    mask = torch.empty(lib().sis_bn_mask_words(b, c, h * w), dtype=torch.int64, device=x.device) if (want_mask and relu) else None
    with torch.cuda.device(x.device):
        _check(lib().sis_bn_act_fwd(_ptr(y), _ptr(x), _ptr(residual), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), b, c,
                                    h * w, int(bool(relu)), _ptr(mask), _stream()), "sis_bn_act_fwd")
    return (y, mask) if want_mask else y


def bn_act_bwd(dy, y, x, mean, invstd, gamma, relu, want_residual_grad, mask=None):
    """``mask`` (from ``bn_act_fwd(..., want_mask=True)``) replaces ``y`` as the ReLU gate (y may be None)."""
    b, c, h, w = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual_grad else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib().sis_bn_workspace_floats(b, c, h * w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        # (kernel name reported by the library: bn_wide_bwd_kernel / bn_fused_bwd_kernel where a channel fits one workgroup, else the
        # three-launch form)
        _check(_launch(None, 0.0, 4.0 * (3 + want_residual_grad) * x.numel(), lambda: lib().sis_bn_act_bwd(
            _ptr(dx), _ptr(dres), _ptr(dgamma), _ptr(dbeta), _ptr(dy), _ptr(y), _ptr(x), _ptr(mean),
            _ptr(invstd), _ptr(gamma), _ptr(ws), b, c, h * w, int(bool(relu)), _ptr(mask), _stream())),
               "sis_bn_act_bwd")
    return dx, dres, dgamma, dbeta


# ------------------------------------------------------------------------------ DocUFCN (csrc/doc_ufcn.hip)


def _dense_f32(t, name):
    """fp32, on the device, already contiguous: the DocUFCN wrappers never copy (a hidden ``.contiguous()`` is an ATen kernel)."""
    require_device(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
        raise RuntimeError(f"{name}: a contiguous, 16-byte aligned float32 tensor is required ({t.dtype}, {tuple(t.stride())})")
    return t


def dconv3x3(x, weight, bias=None, dilation=1):
    """conv2d(x, weight [Cout,Cin,3,3], bias, stride 1, padding = dilation, dilation) on the fp32 MFMA kernel."""
    x, weight = _dense_f32(x, "input"), _dense_f32(weight, "weight")
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    if tuple(weight.shape) != (cout, cin, 3, 3):
        raise RuntimeError(f"dconv3x3: weight {tuple(weight.shape)} does not fit {cin} input channels")
    if bias is not None:
        bias = _dense_f32(bias, "bias")
    out = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("dconv3x3_kernel", 2.0 * b * cout * cin * 9 * h * w, 4.0 * (x.numel() + out.numel()),
                       lambda: lib().sis_dconv3x3(_ptr(out), _ptr(x), _ptr(weight), _ptr(bias), b, cin, cout, h, w, int(dilation),
                                                  _stream())), "sis_dconv3x3")
    return out


def dconv3x3_adjoint(weight):
    """[Cout,Cin,3,3] -> [Cin,Cout,3,3] with the taps rotated by 180 degrees: ``dconv3x3(dy, adjoint)`` is the data gradient."""
    weight = _dense_f32(weight, "weight")
    cout, cin = weight.shape[:2]
    wa = torch.empty((cin, cout, 3, 3), dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        _check(lib().sis_dconv3x3_adjoint(_ptr(wa), _ptr(weight), cin, cout, _stream()), "sis_dconv3x3_adjoint")
    return wa


def dconv3x3_wgrad(grad_output, x, dilation=1, taps=9):
    """dW [Cout,Cin,3,3] (taps 9) or [Cout,Cin,1,1] (taps 1) from dL/dy and x; deterministic."""
    grad_output, x = _dense_f32(grad_output, "grad_output"), _dense_f32(x, "input")
    b, cin, h, w = x.shape
    cout = grad_output.shape[1]
    k = 3 if taps == 9 else 1
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    n_ws = int(lib().sis_dconv3x3_wgrad_workspace_floats(b, cin, cout, h, w, taps))
    ws = torch.empty(max(n_ws, 4), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("dconv3x3_wgrad_kernel", 2.0 * b * cout * cin * taps * h * w, 4.0 * (x.numel() + grad_output.numel()),
                       lambda: lib().sis_dconv3x3_wgrad(_ptr(dw), _ptr(grad_output), _ptr(x), _ptr(ws), n_ws, b, cin, cout, h, w,
                                                        int(dilation), int(taps), _stream())), "sis_dconv3x3_wgrad")
    return dw


def channel_sum(x):
    """[B,C,H,W] -> [C]: the bias gradient of a layer whose output gradient is x (fixed order)."""
    x = _dense_f32(x, "input")
    b, c = x.shape[:2]
    out = torch.empty(c, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_channel_sum(_ptr(out), _ptr(x), b, c, x[0, 0].numel(), _stream()), "sis_channel_sum")
    return out


def pixel_shuffle2(x, bias=None, out=None, channel_offset=0):
    """nn.PixelShuffle(2) (+ per-channel bias) of x [B,4C,H,W] -> [B,C,2H,2W].  ``out``: a contiguous [B, C', 2H, 2W] buffer whose
    channels [channel_offset, channel_offset + C) receive the result (returned)."""
    x = _dense_f32(x, "input")
    b, c4, h, w = x.shape
    c = c4 // 4
    if bias is not None:
        bias = _dense_f32(bias, "bias")
    if out is None:
        out, channel_offset = torch.empty((b, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device), 0
    out = _dense_f32(out, "out")
    if out.shape[0] != b or tuple(out.shape[2:]) != (2 * h, 2 * w) or channel_offset + c > out.shape[1]:
        raise RuntimeError("pixel_shuffle2: output buffer does not fit")
    dst = ctypes.c_void_p(out.data_ptr() + 4 * channel_offset * 4 * h * w)
    with torch.cuda.device(x.device):
        _check(lib().sis_pixel_shuffle2(dst, _ptr(x), _ptr(bias), b, c, h, w, out.shape[1] * 4 * h * w, 0, _stream()),
               "sis_pixel_shuffle2")
    return out


def pixel_shuffle2_grad(g, channels=None, channel_offset=0):
    """Gradient of ``pixel_shuffle2``: channels [channel_offset, channel_offset + channels) of g [B, C', 2H, 2W] -> [B, 4C, H, W]."""
    g = _dense_f32(g, "grad_output")
    b, ctot, h2, w2 = g.shape
    c = ctot - channel_offset if channels is None else channels
    h, w = h2 // 2, w2 // 2
    out = torch.empty((b, 4 * c, h, w), dtype=torch.float32, device=g.device)
    src = ctypes.c_void_p(g.data_ptr() + 4 * channel_offset * h2 * w2)
    with torch.cuda.device(g.device):
        _check(lib().sis_pixel_shuffle2(_ptr(out), src, None, b, c, h, w, ctot * h2 * w2, 1, _stream()), "sis_pixel_shuffle2")
    return out


def max_pool2x2_slice(buf, channel_offset, channels):
    """2x2 / stride-2 max pooling of channels [channel_offset, channel_offset + channels) of a contiguous [B, C', H, W] buffer ->
    (out [B, channels, H/2, W/2], argmax): one ``sis_max_pool2d`` launch per sample (its planes are contiguous there)."""
    buf = _dense_f32(buf, "input")
    b, ctot, h, w = buf.shape
    out = torch.empty((b, channels, h // 2, w // 2), dtype=torch.float32, device=buf.device)
    arg = torch.empty((b, channels, h // 2, w // 2), dtype=torch.uint8, device=buf.device)
    plane_out = channels * (h // 2) * (w // 2)
    with torch.cuda.device(buf.device):
        for i in range(b):
            src = buf.data_ptr() + 4 * (i * ctot + channel_offset) * h * w
            _check(lib().sis_max_pool2d(ctypes.c_void_p(out.data_ptr() + 4 * i * plane_out), ctypes.c_void_p(arg.data_ptr() + i * plane_out),
                                        ctypes.c_void_p(src), F32, channels, h, w, h // 2, w // 2, 2, 2, 0, 0, _stream()),
                   "sis_max_pool2d")
    return out, arg


def transpose2d(x):
    x = _dense_f32(x, "input")
    rows, cols = x.shape
    out = torch.empty((cols, rows), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().sis_transpose2d(_ptr(out), _ptr(x), rows, cols, _stream()), "sis_transpose2d")
    return out


def bn_drop_fwd(x, mean, invstd_or_var, gamma, beta, eval_mode=False, eps=1e-5, seed=None, site=0, drop_p=0.0, out=None,
                channel_offset=0, want_mask=True):
    """y = dropout(relu(bn(x))) -> (y, mask).  ``out``: a wider [B, C', H, W] buffer whose channels
    [channel_offset, channel_offset + C) receive y (returned instead of a fresh tensor)."""
    x = _dense_f32(x, "input")
    b, c, h, w = x.shape
    if out is None:
        out, bstride, y = torch.empty_like(x), c * h * w, None
    else:
        if out.dim() != 4 or tuple(out.shape[2:]) != (h, w) or out.shape[0] != b or not out.is_contiguous() \
                or channel_offset + c > out.shape[1]:
            raise RuntimeError("bn_drop_fwd: out must be a contiguous [B, >= offset + C, H, W] buffer")
        bstride, y = out.shape[1] * h * w, out
    mask = torch.empty(lib().sis_bn_mask_words(b, c, h * w), dtype=torch.int64, device=x.device) if want_mask else None
    dst = out.data_ptr() + 4 * channel_offset * h * w
    with torch.cuda.device(x.device):
        _check(lib().sis_bn_drop_fwd(ctypes.c_void_p(dst), bstride, _ptr(x), _ptr(mean), _ptr(invstd_or_var), _ptr(gamma),
                                     _ptr(beta), b, c, h * w, int(bool(eval_mode)), float(eps), _ptr(seed), int(site),
                                     float(drop_p), _ptr(mask), _stream()), "sis_bn_drop_fwd")
    return (out if y is None else y), mask


def bn_drop_bwd(dy, x, mean, invstd, gamma, mask, drop_p, channel_offset=0, dy2=None):
    """Backward of ``bn_drop_fwd`` -> (dx, dgamma, dbeta).  dy may be a wider [B, C', H, W] buffer whose channels
    [channel_offset, channel_offset + C) are y's gradient; ``dy2`` (contiguous, x's shape) is added to it."""
    x = _dense_f32(x, "input")
    b, c, h, w = x.shape
    if dy is None:
        dy, channel_offset = dy2, 0
        dy2 = None
    dy = _dense_f32(dy, "grad_output")
    if dy.dim() != 4 or dy.shape[0] != b or tuple(dy.shape[2:]) != (h, w) or channel_offset + c > dy.shape[1]:
        raise RuntimeError("bn_drop_bwd: grad_output must be a [B, >= offset + C, H, W] buffer")
    if dy2 is not None:
        dy2 = _dense_f32(dy2, "grad_output")
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib().sis_bn_drop_bwd_workspace_floats(b, c, h * w)), dtype=torch.float32, device=x.device)
    src = dy.data_ptr() + 4 * channel_offset * h * w
    with torch.cuda.device(x.device):
        _check(lib().sis_bn_drop_bwd(_ptr(dx), _ptr(dgamma), _ptr(dbeta), ctypes.c_void_p(src), dy.shape[1] * h * w, _ptr(dy2),
                                     _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(mask), float(drop_p), _ptr(ws), b, c,
                                     h * w, _stream()), "sis_bn_drop_bwd")
    return dx, dgamma, dbeta


def weighted_ce_fwd(logits, labels, weight=None):
    """nn.CrossEntropyLoss(weight=weight)(logits [B,K,H,W], labels [B,H,W] int64) -> (loss [1], stats [1] = sum of weights)."""
    logits, weight = _dense_f32(logits, "logits"), (None if weight is None else _dense_f32(weight, "weight"))
    require_device(labels, "labels")
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise RuntimeError("weighted_ce_fwd: labels must be a contiguous int64 tensor")
    b, k, h, w = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    stats = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = torch.empty(lib().sis_weighted_ce_workspace_floats(), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _check(lib().sis_weighted_ce_fwd(_ptr(loss), _ptr(stats), _ptr(ws), _ptr(logits), _ptr(labels), _ptr(weight), b, k, h * w,
                                         _stream()), "sis_weighted_ce_fwd")
    return loss, stats


def weighted_ce_bwd(grad_loss, logits, labels, weight, stats):
    grad_loss = _dense_f32(grad_loss.reshape(1), "grad_loss")
    b, k, h, w = logits.shape
    grad = torch.empty_like(logits)
    with torch.cuda.device(logits.device):
        _check(lib().sis_weighted_ce_bwd(_ptr(grad), _ptr(grad_loss), _ptr(logits), _ptr(labels), _ptr(weight), _ptr(stats), b, k,
                                         h * w, _stream()), "sis_weighted_ce_bwd")
    return grad


def adam_chunk_elems():
    return int(lib().sis_adam_chunk_elems())


def adam_clip_step(table, n_chunks, partial, hyper, step):
    with torch.cuda.device(table.device):
        _check(lib().sis_adam_clip_step(_ptr(table), int(n_chunks), _ptr(partial), _ptr(hyper), _ptr(step), _stream()),
               "sis_adam_clip_step")


# ------------------------------------------------------------------------------ DatasetGAN pixel-ensemble labelling


def _layer_pair(layers, name):
    """<= 2 contiguous fp32 [B, c, r, r] tensors -> (tensors, host words {act0, act1, c0, c1})."""
    if len(layers) > 2:
        raise RuntimeError(f"{name}: at most two activation layers per resolution group")
    ts = [_dense_f32(t, name) for t in layers]
    words = [0, 0, 0, 0]
    for i, t in enumerate(ts):
        words[i], words[2 + i] = t.data_ptr(), t.shape[1]
    return ts, words


def pixel_ensemble_label(full, groups, w1f, b1, w2t, b2, w3t, b3, classes, hidden1, size, lut=None, want_logits=False):
    """Voted DatasetGAN labels of a batch (csrc/pixel_ensemble.hip).

    full: the full-resolution activation layers ([B, c, S, S], at most two; empty: none) and w1f [sum c][N * hidden1] their
    first-layer weights (k-major); groups: [(layers at one resolution r < S (at most two), wt [sum c][N * hidden1])];
    b1 [N * hidden1]; w2t [N][hidden1][H2], b2 [N][H2], w3t [N][H2][CP], b3 [N][CP] with BatchNorm folded in.
    -> (labels int64 [B, S, S], colours uint8 [B, S, S, 3] when a [C, 3] uint8 lut is given, else None,
        member logits [N, B, S, S, C] when want_logits, else None)."""
    members, m = w2t.shape[0], b1.numel()
    acts = list(full) + [t for layers, _ in groups for t in layers]
    if not acts:
        raise RuntimeError("pixel_ensemble_label: no activations")
    dev, batch = acts[0].device, acts[0].shape[0]
    full_ts, full_words = _layer_pair(full, "full-resolution activations")
    keep, gwords, pwords, projs = [], [], [], []
    for layers, wt in groups:
        ts, words = _layer_pair(layers, "activations")
        res = ts[0].shape[-1]
        wt = _dense_f32(wt, "projection weights")
        out = torch.empty((batch, res * res, m), dtype=torch.float32, device=dev)
        keep += ts + [wt]
        projs.append(out)
        gwords += [res, wt.data_ptr(), out.data_ptr(), words[0], words[1], words[2], words[3]]
        pwords += [out.data_ptr(), res]
    weights = [_dense_f32(t, n) for t, n in ((b1, "b1"), (w2t, "w2t"), (b2, "b2"), (w3t, "w3t"), (b3, "b3"))]
    w1f = _dense_f32(w1f, "w1f") if full_ts else None
    labels = torch.empty((batch, size, size), dtype=torch.int64, device=dev)
    rgb = torch.empty((batch, size, size, 3), dtype=torch.uint8, device=dev) if lut is not None else None
    if lut is not None and (lut.dtype != torch.uint8 or not lut.is_cuda or tuple(lut.shape) != (classes, 3)):
        raise RuntimeError("pixel_ensemble_label: the colour table must be a uint8 [C, 3] device tensor")
    logits = torch.empty((members, batch, size, size, classes), dtype=torch.float32, device=dev) if want_logits else None
    g_arr = (ctypes.c_int64 * max(len(gwords), 1))(*gwords)
    p_arr = (ctypes.c_int64 * max(len(pwords), 1))(*pwords)
    f_arr = (ctypes.c_int64 * 4)(*full_words)
    kf = full_words[2] + full_words[3]
    flops_proj = 2.0 * m * sum(t.shape[1] * t.shape[2] * t.shape[3] for layers, _ in groups for t in layers)
    hidden2, cp = w2t.shape[2], w3t.shape[2]
    flops_head = 2.0 * batch * size * size * (m * kf + members * (hidden1 * hidden2 + hidden2 * cp)) \
        + 8.0 * batch * size * size * m * len(groups)
    with torch.cuda.device(dev):
        if groups:
            _check(_launch("pe_project_kernel", flops_proj, 4.0 * (sum(t.numel() for t in keep) + sum(t.numel() for t in projs)),
                           lambda: lib().sis_pixel_ensemble_project(g_arr, len(groups), batch, m, _stream())),
                   "sis_pixel_ensemble_project")
        _check(_launch(f"pe_head_kernel<{hidden1},{hidden2},{cp}>", flops_head,
                       4.0 * (sum(t.numel() for t in full_ts) * members + sum(t.numel() for t in projs)) + 8.0 * labels.numel(),
                       lambda: lib().sis_pixel_ensemble_head(f_arr, p_arr, len(projs), _ptr(w1f), *[_ptr(t) for t in weights],
                                                             _ptr(lut), _ptr(labels), _ptr(rgb), _ptr(logits), batch, size,
                                                             members, classes, hidden1, _stream())),
               "sis_pixel_ensemble_head")
    return labels, rgb, logits


# ------------------------------------------------------------------------------ DatasetGAN training

PE_TRAIN_HIDDEN = (128, 32)   # the narrow PixelClassifier (2..31 classes); the wide one is not on the fused path
PE_TRAIN_MAX_MEMBERS = 10


def pe_train_workspace_bytes(piece, pixels, features, members):
    """Bytes of the workspace of ``pe_train_tail`` (piece 0) or ``pe_train_l1_wgrad`` (piece 1)."""
    n = lib().sis_pe_train_workspace_bytes(int(piece), int(pixels), int(features), int(members))
    if n < 0:
        raise RuntimeError(f"pe_train: unsupported shape: {pixels} pixels (>= 2), {features} features (a multiple of 32), "
                           f"{members} members (1..{PE_TRAIN_MAX_MEMBERS})")
    return n


def _pe_workspace(workspace, nbytes, device):
    if workspace is None:
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    if workspace.dtype != torch.uint8 or workspace.numel() < nbytes or workspace.device != device or workspace.data_ptr() % 256:
        raise RuntimeError(f"pe_train: the workspace must be a 256-byte aligned uint8 device tensor of at least {nbytes} bytes")
    return workspace


def pe_train_layer_table(layers):
    """(host words, device int64 [L, 4]) of resident activation layers [images, c, res, res] in feature order: {pointer, c, res,
    first column} per layer.  Keep the layers alive as long as the table is used."""
    words, col = [], 0
    for t in layers:
        require_device(t, "activations")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4 or t.shape[2] != t.shape[3]:
            raise RuntimeError("pe_train: activation layers must be contiguous float32 [images, c, res, res]")
        words += [t.data_ptr(), t.shape[1], t.shape[2], col]
        col += t.shape[1]
    return words, torch.tensor(words, dtype=torch.int64).view(-1, 4).to(layers[0].device)


def pe_train_gather(layers, pixels, size, table=None, out=None):
    """X [P, F]: the DatasetGAN features of P pixels (int32 [P, 3] = image, y, x) of resident activation layers
    [images, c, res, res], bilinear with align_corners=False as the label pass samples them (csrc/pixel_ensemble_train.h)."""
    require_device(pixels, "pixels")
    if pixels.dtype != torch.int32 or pixels.dim() != 2 or pixels.shape[1] != 3 or not pixels.is_contiguous():
        raise RuntimeError("pe_train_gather: pixels must be a contiguous int32 [P, 3] tensor")
    words, dev_table = table if table is not None else pe_train_layer_table(layers)
    npix, features, images = pixels.shape[0], sum(t.shape[1] for t in layers), layers[0].shape[0]
    if any(t.shape[0] != images for t in layers):
        raise RuntimeError("pe_train_gather: the layers hold different numbers of images")
    if out is None:
        out = torch.empty((npix, features), dtype=torch.float32, device=pixels.device)
    host = (ctypes.c_int64 * len(words))(*words)
    with torch.cuda.device(pixels.device):
        _check(_launch("pe_gather_kernel", 7.0 * npix * features, 20.0 * npix * features,
                       lambda: lib().sis_pe_train_gather(host, _ptr(dev_table), len(layers), _ptr(pixels), _ptr(out), npix, features,
                                                         int(size), images, _stream())), "sis_pe_train_gather")
    return out


def pe_train_l1_forward(x, w1, b1, out=None):
    """a1 [P, N*128] = relu(x w1^T + b1) for x [P, F], w1 [N*128, F] (the members' first layers stacked)."""
    x, w1, b1 = _dense_f32(x, "x"), _dense_f32(w1, "w1"), _dense_f32(b1, "b1")
    npix, features = x.shape
    m = w1.shape[0]
    if m % PE_TRAIN_HIDDEN[0] or tuple(w1.shape) != (m, features) or b1.numel() != m:
        raise RuntimeError("pe_train_l1_forward: w1 must be [N*128, F] and b1 [N*128]")
    if out is None:
        out = torch.empty((npix, m), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("pe_l1_fwd_kernel", 2.0 * npix * features * m, 4.0 * (x.numel() + w1.numel() + out.numel()),
                       lambda: lib().sis_pe_train_l1_forward(_ptr(x), _ptr(w1), _ptr(b1), _ptr(out), npix, features,
                                                             m // PE_TRAIN_HIDDEN[0], _stream())), "sis_pe_train_l1_forward")
    return out


PE_TRAIN_PARAMS = ("g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3")
PE_TRAIN_RUNNING = ("mean1", "var1", "mean2", "var2", "tracked1", "tracked2")


def pe_train_tail(a1, labels, params, classes, running=None, grads=None, dz1=None, loss=None, want_logits=False, workspace=None):
    """Everything between the first layer's output and its gradient, for N members at once (csrc/pixel_ensemble_train.h).

    a1 [P, N*128] (after ReLU); labels int64 [P]; params: dict of PE_TRAIN_PARAMS (g1 / be1 [N*128], w2 [N, 32, 128], b2 / g2 / be2
    [N*32], w3 [N, C, 32], b3 [N, C]); running: dict with any of PE_TRAIN_RUNNING, updated in place (tracked: int64 [N]).
    -> {"dz1": [P, N*128], "loss": [N], "grads": {d + name}, "logits": [N, P, C] or None}."""
    a1 = _dense_f32(a1, "a1")
    require_device(labels, "labels")
    npix, m = a1.shape
    h1, h2 = PE_TRAIN_HIDDEN
    members = m // h1
    if m % h1 or labels.dtype != torch.int64 or labels.numel() != npix or not labels.is_contiguous():
        raise RuntimeError("pe_train_tail: a1 must be [P, N*128] and labels a contiguous int64 [P] tensor")
    shapes = {"g1": m, "be1": m, "w2": members * h2 * h1, "b2": members * h2, "g2": members * h2, "be2": members * h2,
              "w3": members * classes * h2, "b3": members * classes}
    ps = [_dense_f32(params[k], k) for k in PE_TRAIN_PARAMS]
    for k, t in zip(PE_TRAIN_PARAMS, ps):
        if t.numel() != shapes[k]:
            raise RuntimeError(f"pe_train_tail: {k} has {t.numel()} elements, expected {shapes[k]}")
    nbytes = pe_train_workspace_bytes(0, npix, 32, members)
    dev = a1.device
    workspace = _pe_workspace(workspace, nbytes, dev)
    if grads is None:
        grads = {"d" + k: torch.empty(tuple(params[k].shape), dtype=torch.float32, device=dev) for k in PE_TRAIN_PARAMS}
    gs = [grads["d" + k] for k in PE_TRAIN_PARAMS]
    for k, t in zip(PE_TRAIN_PARAMS, gs):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != shapes[k] or t.device != dev:
            raise RuntimeError(f"pe_train_tail: gradient d{k} must be a contiguous float32 tensor of {shapes[k]} elements")
    running = running or {}
    rs = []
    for k in PE_TRAIN_RUNNING:
        t = running.get(k)
        if t is not None:
            want = torch.int64 if k.startswith("tracked") else torch.float32
            count = members if k.startswith("tracked") else (m if k.endswith("1") else members * h2)
            if t.dtype != want or not t.is_contiguous() or t.numel() != count or t.device != dev:
                raise RuntimeError(f"pe_train_tail: running['{k}'] must be a contiguous {want} tensor of {count} elements")
        rs.append(t)
    if dz1 is None:
        dz1 = torch.empty((npix, m), dtype=torch.float32, device=dev)
    if loss is None:
        loss = torch.empty((members,), dtype=torch.float32, device=dev)
    logits = torch.empty((members, npix, classes), dtype=torch.float32, device=dev) if want_logits else None
    c_params = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ps])
    c_grads = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in gs])
    c_running = (ctypes.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in rs])
    flops = 2.0 * npix * members * 3 * (h1 * h2 + h2 * classes)
    with torch.cuda.device(dev):
        _check(_launch("pe_train_tail", flops, 4.0 * 4 * a1.numel(),
                       lambda: lib().sis_pe_train_tail(_ptr(a1), _ptr(labels), c_params, c_running, c_grads, _ptr(dz1), _ptr(loss),
                                                       _ptr(logits), _ptr(workspace), npix, members, int(classes), _stream())),
               "sis_pe_train_tail")
    return {"dz1": dz1, "loss": loss, "grads": grads, "logits": logits}


def pe_train_l1_wgrad(dz1, x, dw1=None, db1=None, workspace=None):
    """(dw1 [N*128, F] = dz1^T x, db1 [N*128] = column sums of dz1) for dz1 [P, N*128], x [P, F]."""
    dz1, x = _dense_f32(dz1, "dz1"), _dense_f32(x, "x")
    npix, m = dz1.shape
    features = x.shape[1]
    if m % PE_TRAIN_HIDDEN[0] or x.shape[0] != npix:
        raise RuntimeError("pe_train_l1_wgrad: dz1 must be [P, N*128] and x [P, F]")
    members = m // PE_TRAIN_HIDDEN[0]
    if features % 32 or not 1 <= members <= PE_TRAIN_MAX_MEMBERS:
        raise RuntimeError(f"pe_train_l1_wgrad: {features} features (a multiple of 32), {members} members (1..{PE_TRAIN_MAX_MEMBERS})")
    nbytes = lib().sis_pe_train_workspace_bytes(1, max(npix, 2), features, members)
    workspace = _pe_workspace(workspace, nbytes, x.device)
    if dw1 is None:
        dw1 = torch.empty((m, features), dtype=torch.float32, device=x.device)
    if db1 is None:
        db1 = torch.empty((m,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("pe_l1_wgrad_kernel", 2.0 * npix * features * m, 4.0 * (x.numel() + dz1.numel() + dw1.numel()),
                       lambda: lib().sis_pe_train_l1_wgrad(_ptr(dz1), _ptr(x), _ptr(dw1), _ptr(db1), _ptr(workspace), npix, features,
                                                           members, _stream())), "sis_pe_train_l1_wgrad")
    return dw1, db1


# ------------------------------------------------------------------------------ training-time augmentation

ELASTIC_MAX_FIELDS = 64   # per launch of sis_elastic_field; the binding splits longer lists
ELASTIC_MAX_SIGMA = 9.0


def elastic_radius(sigma):
    """floor(4 sigma + 0.5) in float32, the filter radius the kernel uses (scipy: int(truncate * sigma + 0.5))."""
    import numpy
    return int(numpy.float32(4.0) * numpy.float32(sigma) + numpy.float32(0.5))


def elastic_field(height, width, sigma, alpha, seeds=None, noise=None, device=None, return_noise=False):
    """Displacement fields [F, 2, H, W] float32 (component 0 = x) for F = len(sigma) elastic draws: alpha * (Gaussian of sigma,
    mirror boundary, radius floor(4 sigma + 0.5)) * noise.  ``seeds``: F 32-bit words for the counter hash of DESIGN.md §12;
    ``noise``: a float32 [F, 2, H, W] device tensor to blur instead (tests).  An image that is not larger than a filter radius,
    or a sigma above 9, is refused with ``ValueError`` before anything is launched."""
    sigma, alpha = [float(v) for v in sigma], [float(v) for v in alpha]
    n = len(sigma)
    if n == 0 or len(alpha) != n:
        raise ValueError("elastic_field: one alpha per sigma, at least one field")
    for sg in sigma:
        if not 0.0 < sg <= ELASTIC_MAX_SIGMA:
            raise ValueError(f"elastic_field: sigma {sg} outside (0, {ELASTIC_MAX_SIGMA}]")
        if min(height, width) <= elastic_radius(sg):
            raise ValueError(f"elastic_field: a {height}x{width} image is not larger than the filter radius "
                             f"{elastic_radius(sg)} of sigma {sg}")
    if noise is not None:
        noise = _f32(noise, "noise")
        if tuple(noise.shape) != (n, 2, height, width):
            raise RuntimeError(f"noise must be [{n}, 2, {height}, {width}], got {tuple(noise.shape)}")
        device = noise.device
    elif seeds is None or len(seeds) != n:
        raise ValueError("elastic_field: one seed word per field, or a noise tensor")
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError("device must be a CUDA tensor")
    field = torch.empty((n, 2, height, width), dtype=torch.float32, device=device)
    ws = torch.empty_like(field)
    used = torch.empty_like(field) if return_noise else None
    with torch.cuda.device(device):
        for lo in range(0, n, ELASTIC_MAX_FIELDS):
            m = min(ELASTIC_MAX_FIELDS, n - lo)
            c_alpha, c_sigma = (ctypes.c_float * m)(*alpha[lo:lo + m]), (ctypes.c_float * m)(*sigma[lo:lo + m])
            c_seeds = None if seeds is None else (ctypes.c_uint32 * m)(*[int(v) & 0xFFFFFFFF for v in seeds[lo:lo + m]])
            _check(_launch("elastic_field", 0.0, 16.0 * m * 2 * height * width,
                           lambda: lib().sis_elastic_field(_ptr(field[lo:]), _ptr(ws[lo:]), None if used is None else _ptr(used[lo:]),
                                                           None if noise is None else _ptr(noise[lo:]), c_alpha, c_sigma, c_seeds,
                                                           m, height, width, _stream())), "sis_elastic_field")
    return (field, used) if return_noise else field


def augment_warp(pixels, classes, index, minv, lut, field_slot, field=None, background_id=0, out_size=None, quantize=True):
    """One batch of the reference loaders' contract from the resident dataset (csrc/augment.hip): pixels uint8
    [N, H, W, 3], classes uint8 [N, H, W], index int32 [B], minv float32 [B, 2, 3], lut uint8 [B, 256], field_slot int32 [B]
    (-1: no elastic), field float32 [F, 2, H, W] or None, all on one device -> {"images": float32 [B, 3, S, S], "segmented":
    int64 [B, 1, S, S]}.  ``out_size``: S, or (height, width); default: the source size."""
    for t, name, dtype in ((pixels, "pixels", torch.uint8), (classes, "classes", torch.uint8), (index, "index", torch.int32),
                           (minv, "minv", torch.float32), (lut, "lut", torch.uint8), (field_slot, "field_slot", torch.int32)):
        require_device(t, name)
        if t.dtype != dtype or not t.is_contiguous() or t.device != pixels.device:
            raise RuntimeError(f"{name} must be a contiguous {dtype} tensor on the device of pixels")
    if pixels.dim() != 4 or pixels.shape[3] != 3 or tuple(classes.shape) != tuple(pixels.shape[:3]):
        raise RuntimeError("pixels must be [N, H, W, 3] and classes [N, H, W]")
    n, h, w, _ = pixels.shape
    b = index.numel()
    if tuple(minv.shape) != (b, 2, 3) or tuple(lut.shape) != (b, 256) or field_slot.numel() != b:
        raise RuntimeError("minv must be [B, 2, 3], lut [B, 256] and field_slot [B] for index [B]")
    num_fields = 0
    if field is not None:
        field = _f32(field, "field")
        if field.dim() != 4 or tuple(field.shape[1:]) != (2, h, w) or field.device != pixels.device:
            raise RuntimeError(f"field must be [F, 2, {h}, {w}] on the device of pixels")
        num_fields = field.shape[0]
    if out_size is None:
        out_h, out_w = h, w
    elif isinstance(out_size, int):
        out_h = out_w = out_size
    else:
        out_h, out_w = (int(v) for v in out_size)
    images = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=pixels.device)
    segmented = torch.empty((b, 1, out_h, out_w), dtype=torch.int64, device=pixels.device)
    with torch.cuda.device(pixels.device):
        # per output pixel: 12 + 8 bytes written, 4 taps of 3 source bytes and 1 class byte read (fields: 8 more taps of 4 bytes)
        _check(_launch("augment_warp_kernel", 0.0, 33.0 * images.numel() / 3,
                       lambda: lib().sis_augment_warp(_ptr(images), _ptr(segmented), _ptr(pixels), _ptr(classes), _ptr(index),
                                                      _ptr(minv), _ptr(lut), _ptr(field_slot), _ptr(field), n, b, h, w, num_fields,
                                                      int(background_id), out_h, out_w, int(bool(quantize)), _stream())),
               "sis_augment_warp")
    return {"images": images, "segmented": segmented}


# ------------------------------------------------------------------------------ projection encoders (csrc/encoder_ops.h)


def fold_batch_norm(bn, conv_bias=None):
    """Eval-mode BatchNorm2d as (scale, shift) float32 [C]: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
    (+ scale * conv_bias: the bias of the convolution in front of it).  Computed in float64, rounded once."""
    var, mean = bn.running_var.detach().double(), bn.running_mean.detach().double()
    scale = torch.rsqrt(var + bn.eps)
    if bn.weight is not None:
        scale = scale * bn.weight.detach().double()
    shift = -mean * scale
    if bn.bias is not None:
        shift = shift + bn.bias.detach().double()
    if conv_bias is not None:
        shift = shift + scale * conv_bias.detach().double()
    return scale.float().contiguous(), shift.float().contiguous()


def enc_conv3x3_s2_supported(cin, cout, h, w):
    return bool(lib().sis_enc_conv3x3_s2_supported(int(cin), int(cout), int(h), int(w)))


def enc_conv3x3_s2_pack(weight, shortcut_weight=None):
    """[Cout, Cin, 3, 3] (+ the block's 1x1 stride-2 shortcut weight [Cout, Cin, 1, 1]) -> the k-major image of
    ``enc_conv3x3_s2``: [Cin, 9 or 10, Cout padded to 64]."""
    w = _f32(weight, "weight")
    cout, cin = w.shape[0], w.shape[1]
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("enc_conv3x3_s2_pack: a [Cout, Cin, 3, 3] weight is needed")
    wd = None
    if shortcut_weight is not None:
        wd = _f32(shortcut_weight, "shortcut weight")
        if wd.numel() != cout * cin:
            raise RuntimeError("enc_conv3x3_s2_pack: the shortcut weight must be [Cout, Cin, 1, 1]")
    taps = 10 if wd is not None else 9
    packed = torch.empty((cin, taps, -(-cout // 64) * 64), dtype=torch.float32, device=w.device)
    assert packed.numel() == lib().sis_enc_conv3x3_s2_packed_floats(cin, cout, int(wd is not None))
    with torch.cuda.device(w.device):
        _check(_launch("enc_conv3x3_s2_prepack", 0.0, 4.0 * (w.numel() + packed.numel()),
                       lambda: lib().sis_enc_conv3x3_s2_pack(_ptr(packed), _ptr(w), _ptr(wd), cin, cout, _stream())), "sis_enc_conv3x3_s2_pack")
    return packed


def enc_conv3x3_s2(x, packed, cout, scale1, shift1, scale_d=None, shift_d=None):
    """relu(scale1 * conv3x3_stride2_pad1(x) + shift1) and, with scale_d / shift_d (``packed`` then holds the shortcut
    weights), scale_d * conv1x1_stride2(x) + shift_d from the same read of x -> (y_main, y_short or None)."""
    x = _f32(x, "input")
    batch, cin, h, w = x.shape
    short = scale_d is not None
    if packed.shape[0] != cin or packed.shape[1] != (10 if short else 9) or packed.shape[2] != -(-cout // 64) * 64:
        raise RuntimeError(f"enc_conv3x3_s2: packed weights {tuple(packed.shape)} do not fit {cin} -> {cout} channels"
                           f"{' with a shortcut' if short else ''}")
    y = torch.empty((batch, cout, h // 2, w // 2), dtype=torch.float32, device=x.device)
    ys = torch.empty((batch, cout, h // 2, w // 2), dtype=torch.float32, device=x.device) if short else None
    flops = 2.0 * batch * cout * cin * (10 if short else 9) * (h // 2) * (w // 2)
    with torch.cuda.device(x.device):
        _check(_launch("enc_conv3x3_s2_kernel", flops, 4.0 * (x.numel() + (2 if short else 1) * y.numel() + packed.numel()),
                       lambda: lib().sis_enc_conv3x3_s2(_ptr(y), _ptr(ys), _ptr(x), _ptr(packed), _ptr(scale1), _ptr(shift1), _ptr(scale_d),
                                                        _ptr(shift_d), batch, cin, cout, h, w, _stream())), "sis_enc_conv3x3_s2")
    return y, ys


def enc_stem_supported(cin, cout, h, w):
    return bool(lib().sis_enc_stem_supported(int(cin), int(cout), int(h), int(w)))


def enc_stem(x, weight, scale1, shift1, shortcut_weight, shortcut_bias, scale_d, shift_d):
    """The start block from <= 4 input channels: (relu(scale1 * conv3x3(x) + shift1), scale_d * (conv1x1(x) + bias) + shift_d)."""
    x, w1, wd = _f32(x, "input"), _f32(weight, "weight"), _f32(shortcut_weight, "shortcut weight")
    batch, cin, h, w = x.shape
    cout = w1.shape[0]
    if tuple(w1.shape) != (cout, cin, 3, 3) or wd.numel() != cout * cin:
        raise RuntimeError("enc_stem: weights must be [Cout, Cin, 3, 3] and [Cout, Cin, 1, 1]")
    y = torch.empty((batch, cout, h, w), dtype=torch.float32, device=x.device)
    ys = torch.empty((batch, cout, h, w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(_launch("enc_stem_kernel", 2.0 * batch * cout * cin * 10 * h * w, 4.0 * (x.numel() + 2 * y.numel()),
                       lambda: lib().sis_enc_stem(_ptr(y), _ptr(ys), _ptr(x), _ptr(w1), _ptr(wd), _ptr(shortcut_bias), _ptr(scale1), _ptr(shift1),
                                                  _ptr(scale_d), _ptr(shift_d), batch, cin, cout, h, w, _stream())), "sis_enc_stem")
    return y, ys


def enc_block_tail_supported(channels, hw):
    return bool(lib().sis_enc_block_tail_supported(int(channels), int(hw)))


def enc_block_tail_tiles(hw):
    return int(lib().sis_enc_block_tail_tiles(int(hw)))


def enc_block_tail(c, residual, scale, shift, noise_weight=None, noise_bias=None, want_pool=False, pool_out=None):
    """y = relu(scale * c + shift + residual) -> (y, noise [B,1,H,W] or None, pool partials [B,C,tiles] or None);
    ``noise_weight`` [1,C,1,1] / ``noise_bias`` [1]: the 1x1 convolution of y to one channel; ``want_pool``: per-tile sums of y
    (``sis_enc_latent_heads`` finishes the average), written into ``pool_out`` when given."""
    c = _f32(c, "input")
    batch, ch, h, w = c.shape
    hw = h * w
    if residual is not None:
        residual = _f32(residual, "residual")
        if residual.shape != c.shape:
            raise RuntimeError("enc_block_tail: the residual must have the input's shape")
    y = torch.empty((batch, ch, h, w), dtype=torch.float32, device=c.device)
    noise = torch.empty((batch, 1, h, w), dtype=torch.float32, device=c.device) if noise_weight is not None else None
    partial = None
    if want_pool:
        tiles = enc_block_tail_tiles(hw)
        partial = pool_out if pool_out is not None else torch.empty((batch, ch, tiles), dtype=torch.float32, device=c.device)
        if tuple(partial.shape) != (batch, ch, tiles) or partial.dtype != torch.float32 or not partial.is_contiguous():
            raise RuntimeError(f"enc_block_tail: pool_out must be a contiguous float32 [{batch}, {ch}, {tiles}] tensor")
    nw = _f32(noise_weight, "noise weight") if noise_weight is not None else None
    if nw is not None and nw.numel() != ch:
        raise RuntimeError("enc_block_tail: the noise weight must be [1, C, 1, 1]")
    nws = None
    if nw is not None:
        floats = lib().sis_enc_block_tail_workspace_floats(batch, ch, hw)
        nws = torch.empty(floats, dtype=torch.float32, device=c.device) if floats else None   # the channel slices' noise sums
    streams = 2 + (residual is not None)
    with torch.cuda.device(c.device):
        _check(_launch("enc_block_tail_kernel", 0.0, 4.0 * streams * c.numel(),
                       lambda: lib().sis_enc_block_tail(_ptr(y), _ptr(noise), _ptr(partial), _ptr(c), _ptr(residual), _ptr(scale), _ptr(shift),
                                                        _ptr(nw), _ptr(noise_bias), _ptr(nws), batch, ch, hw, _stream())), "sis_enc_block_tail")
    return y, noise, partial


ENC_HEAD_COLS = 8


class EncHeadsTable:
    """The pointer table of ``enc_latent_heads`` with what the launch must know about it: ``table`` int64 [n, 8] on the device,
    ``max_channels`` (the largest C of its rows), ``slots`` (each head's output row) and the tensors it points into."""

    def __init__(self, heads, device):
        rows, self.slots, self.max_channels, self.batch, self.latent = [], [], 0, None, None
        for partial, hw, weight, bias, slot in heads:
            b, ch, tiles = partial.shape
            if weight.dtype != torch.float32 or bias.dtype != torch.float32 or partial.dtype != torch.float32 \
                    or not (weight.is_contiguous() and bias.is_contiguous() and partial.is_contiguous()):
                raise RuntimeError("enc_heads_table: contiguous float32 tensors only")
            for t in (partial, weight, bias):
                require_device(t, "head tensor")
            if weight.numel() != bias.numel() * ch or tiles != enc_block_tail_tiles(hw):
                raise RuntimeError("enc_heads_table: a head needs weight [latent, C], bias [latent] and partials [B, C, tiles of hw]")
            if self.batch not in (None, b) or self.latent not in (None, bias.numel()) or int(slot) < 0:
                raise RuntimeError("enc_heads_table: the heads must share the batch and the latent size; slots are >= 0")
            self.batch, self.latent = b, bias.numel()
            self.max_channels = max(self.max_channels, ch)
            self.slots.append(int(slot))
            rows.append([partial.data_ptr(), weight.data_ptr(), bias.data_ptr(), ch, tiles, int(hw), int(slot), 0])
        if not rows:
            raise RuntimeError("enc_heads_table: no heads")
        self.keep = [t for h in heads for t in (h[0], h[2], h[3])]   # the table holds their addresses
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)


def enc_heads_table(heads, device):
    """``EncHeadsTable`` for ``enc_latent_heads``: one row per head from (partials [B,C,tiles], hw, weight [latent,C(,1,1)],
    bias [latent], slot).  The tensors must stay in place while the table is used."""
    return EncHeadsTable(heads, device)


def enc_latent_heads(heads, n_slots=None, sum_heads=False):
    """Every to_latent head of an encode in one launch -> [B, n_slots, latent] (row ``slot`` of each head; every row must be some
    head's, or it stays unwritten: ``n_slots`` defaults to the number of heads), or with ``sum_heads`` [B, latent]: the sum of
    all heads in table order."""
    if not isinstance(heads, EncHeadsTable):
        raise RuntimeError("enc_latent_heads: the table comes from enc_heads_table")
    table, batch, latent = heads.table, heads.batch, heads.latent
    slots = 1 if sum_heads else int(len(heads.slots) if n_slots is None else n_slots)
    if not sum_heads and (max(heads.slots) >= slots or len(set(heads.slots)) != len(heads.slots)):
        raise RuntimeError(f"enc_latent_heads: slots {heads.slots} do not fit {slots} distinct output rows")
    if not lib().sis_enc_latent_heads_supported(heads.max_channels, latent):
        raise RuntimeError(f"enc_latent_heads: {heads.max_channels} channels with latent size {latent} do not fit the kernel")
    out = torch.empty((batch, slots, latent), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _check(_launch("enc_latent_heads_kernel", 0.0, 0.0,
                       lambda: lib().sis_enc_latent_heads(_ptr(out), _ptr(table), table.shape[0], batch, latent, slots, int(bool(sum_heads)),
                                                          heads.max_channels, _stream())), "sis_enc_latent_heads")
    return out.view(batch, latent) if sum_heads else out


# ------------------------------------------------------------------------------ GAN training (csrc/gan_train_ops.h)


def gan_image_batch(images, ids):
    """Resident uint8 [N, 3, S, S] and int32 ids [B] (both on the device) -> float32 [B, 3, S, S] = (v / 255 - 0.5) / 0.5, the
    reference loader's ToTensor + Normalize(0.5, 0.5) of the listed samples.  The caller keeps the ids inside 0 .. N - 1 (an id
    outside yields a NaN sample)."""
    require_device(images, "images")
    require_device(ids, "ids")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise RuntimeError(f"gan_image_batch: uint8 [N, 3, S, S] images are needed, got {images.dtype} {tuple(images.shape)}")
    if ids.dtype != torch.int32 or ids.dim() != 1 or ids.numel() == 0 or ids.device != images.device:
        raise RuntimeError("gan_image_batch: int32 [B] ids on the images' device are needed")
    images, ids = images.contiguous(), ids.contiguous()
    n, _, size, _ = images.shape
    out = torch.empty((ids.numel(), 3, size, size), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        _check(_launch("gan_image_batch_kernel", 0.0, 5.0 * out.numel(),
                       lambda: lib().sis_gan_image_batch(_ptr(out), _ptr(images), _ptr(ids), n, ids.numel(), size, _stream())),
               "sis_gan_image_batch")
    return out


def phase_split_supported(h, w):
    return bool(lib().sis_phase_split_supported(int(h), int(w)))


def phase_split(x):
    """[B, C, H, W] -> [B, 4C, H/2, W/2], channel order (c, py, px): ``F.pixel_unshuffle(x, 2)``."""
    x = _f32(x, "input")
    if x.dim() != 4 or not phase_split_supported(x.shape[2], x.shape[3]):
        raise RuntimeError(f"phase_split: a [B, C, H, W] tensor with even H and W is needed, got {tuple(x.shape)}")
    b, c, h, w = x.shape
    out = torch.empty((b, 4 * c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    if x.numel():
        with torch.cuda.device(x.device):
            _check(_launch("phase_split_kernel", 0.0, 8.0 * x.numel(),
                           lambda: lib().sis_phase_split(_ptr(out), _ptr(x), b, c, h, w, _stream())), "sis_phase_split")
    return out


def phase_merge(phases):
    """[B, 4C, H/2, W/2] -> [B, C, H, W]: ``F.pixel_shuffle(phases, 2)``, the inverse and the adjoint of ``phase_split``."""
    p = _f32(phases, "phases")
    if p.dim() != 4 or p.shape[1] % 4:
        raise RuntimeError(f"phase_merge: a [B, 4C, H/2, W/2] tensor is needed, got {tuple(p.shape)}")
    b, c4, h2, w2 = p.shape
    out = torch.empty((b, c4 // 4, 2 * h2, 2 * w2), dtype=torch.float32, device=p.device)
    if p.numel():
        with torch.cuda.device(p.device):
            _check(_launch("phase_split_kernel", 0.0, 8.0 * p.numel(),
                           lambda: lib().sis_phase_merge(_ptr(out), _ptr(p), b, c4 // 4, 2 * h2, 2 * w2, _stream())), "sis_phase_merge")
    return out


def down_weight_compose_supported(fir):
    """True for the 4 x 4 FIR (the [1, 3, 3, 1] blur of every discriminator layer); other tap counts stay on blur + library."""
    return fir.dim() == 2 and bool(lib().sis_down_weight_compose_supported(int(fir.shape[0]), int(fir.shape[1])))


def _down_weight_args(weight, fir, channels_factor, what):
    w, f = _f32(weight, what), _f32(fir, "fir")
    if not down_weight_compose_supported(f):
        raise RuntimeError(f"{what}: a {tuple(f.shape)} FIR is not supported (4 x 4 only)")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] % channels_factor or f.device != w.device:
        raise RuntimeError(f"{what}: a [Cout, {'4 Cin' if channels_factor == 4 else 'Cin'}, 3, 3] weight on the FIR's device is needed, "
                           f"got {tuple(w.shape)}")
    return w, f


def down_weight_compose(weight, fir, scale):
    """W [Cout, Cin, 3, 3], normalised FIR taps [4, 4], scale -> W' [Cout, 4 Cin, 3, 3]: Blur(pad 2) + stride-2 convolution with
    scale * W as a stride-1 padding-1 convolution over the ``phase_split`` of the layer's input."""
    w, f = _down_weight_args(weight, fir, 1, "down_weight_compose")
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty((cout, 4 * cin, 3, 3), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _check(_launch("down_weight_compose_kernel", 2.0 * 36 * 9 * cout * cin, 4.0 * (w.numel() + out.numel()),
                       lambda: lib().sis_down_weight_compose(_ptr(out), _ptr(w), _ptr(f), 4, 4, float(scale), cout, cin, _stream())),
               "sis_down_weight_compose")
    return out


def down_weight_compose_adjoint(grad_phases, fir, scale):
    """dW' [Cout, 4 Cin, 3, 3] -> dW [Cout, Cin, 3, 3]: the transpose of ``down_weight_compose`` (scale included)."""
    g, f = _down_weight_args(grad_phases, fir, 4, "down_weight_compose_adjoint")
    cout, cin = g.shape[0], g.shape[1] // 4
    out = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _check(_launch("down_weight_adjoint_kernel", 2.0 * 16 * 9 * cout * cin, 4.0 * (g.numel() + out.numel()),
                       lambda: lib().sis_down_weight_compose_adjoint(_ptr(out), _ptr(g), _ptr(f), 4, 4, float(scale), cout, cin, _stream())),
               "sis_down_weight_compose_adjoint")
    return out


# ------------------------------------------------------------------------------ PNG pairs (csrc/png_encode.h)


def png_capacity(height, width_total):
    """Bytes per image of the output buffer of ``png_encode_pairs`` (the largest file the format can produce, rounded to 16)."""
    return int(lib().sis_png_capacity(int(height), int(width_total)))


def png_ihdr_crc(width_total, height):
    """CRC-32 of the IHDR chunk of an 8-bit RGB image: it depends on the two sizes only, so the host computes it."""
    import struct
    import zlib
    return zlib.crc32(b"IHDR" + struct.pack(">IIBBBBB", int(width_total), int(height), 8, 2, 0, 0, 0))


def png_encode_pairs(image_u8, label_u8=None, out=None):
    """uint8 [N, H, W, 3] images and, optionally, uint8 [N, H, Wl, 3] labels (device) -> (buffer uint8 [N, stride], sizes int32
    [N]): ``buffer[i, :sizes[i]]`` is the complete PNG file of ``[image i | label i]`` (the reference's save_image of the
    concatenated pair, create_dataset_for_segmentation.py:84-90), encoded on the device; the pair itself is never put together.
    ``out``: a contiguous uint8 [N, stride] buffer to write into, stride >= ``png_capacity(H, W + Wl)`` and a multiple of 16."""
    require_device(image_u8, "image")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[3] != 3:
        raise RuntimeError(f"png_encode_pairs: uint8 [N, H, W, 3] images are needed, got {image_u8.dtype} {tuple(image_u8.shape)}")
    image_u8 = image_u8.contiguous()
    n, h, w, _ = image_u8.shape
    wl = 0
    if label_u8 is not None:
        require_device(label_u8, "label")
        if label_u8.dtype != torch.uint8 or label_u8.dim() != 4 or label_u8.shape[3] != 3 or label_u8.shape[:2] != image_u8.shape[:2] \
                or label_u8.device != image_u8.device:
            raise RuntimeError(f"png_encode_pairs: uint8 [{n}, {h}, Wl, 3] labels on the images' device are needed, got {label_u8.dtype} "
                               f"{tuple(label_u8.shape)}")
        label_u8 = label_u8.contiguous()
        wl = label_u8.shape[2]
    stride = png_capacity(h, w + wl)
    if out is None:
        out = torch.empty((n, stride), dtype=torch.uint8, device=image_u8.device)   # (the entry clears it)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n or not out.is_contiguous() or out.device != image_u8.device:
        raise RuntimeError(f"png_encode_pairs: out must be a contiguous uint8 [{n}, stride] tensor on the images' device")
    sizes = torch.empty((n,), dtype=torch.int32, device=image_u8.device)
    ws_bytes = lib().sis_png_encode_pairs_workspace_bytes(n, h)
    ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.int32, device=image_u8.device)
    with torch.cuda.device(image_u8.device):
        _check(_launch("png_emit_kernel", 0.0, 2.0 * 3 * n * h * (w + wl) + 2.0 * out.numel(),   # rows read twice; memset + files
                       lambda: lib().sis_png_encode_pairs(_ptr(out), _ptr(sizes), _ptr(image_u8), _ptr(label_u8), n, h, w, wl, out.shape[1],
                                                          png_ihdr_crc(w + wl, h), _ptr(ws), ws.numel() * 4, _stream())),
               "sis_png_encode_pairs")
    return out, sizes


# ------------------------------------------------------------------------------ reconstruction metrics (csrc/eval_ops.h)

UNNORMALIZE_AUTO, UNNORMALIZE_ALWAYS, UNNORMALIZE_NEVER = 0, 1, 2


def psnr_ssim_tile():
    """Tile edge of the SSIM kernel."""
    return int(lib().sis_psnr_ssim_tile())


def psnr_ssim(image, target, window=5, max_val=1.0, unnormalize=UNNORMALIZE_AUTO, return_map=False):
    """float32 [B, C, H, W] image and target -> (psnr [B], ssim [B]) device tensors, with ``return_map`` also the unclamped SSIM
    map [B, C, H, W]: the reference's ``PSNRSSIMEvaluator`` applied to every sample on its own (DESIGN.md §15 states the
    definitions).  ``psnr`` is the positive metric 10 log10(max_val^2 / mse) (+inf for equal samples), ``ssim`` the mean of
    clamp(s, 0, 1).  ``unnormalize``: 0 decides per sample and tensor by ``min < 0`` as the reference does, 1 maps both tensors
    by (clamp(x, -1, 1) + 1) / 2, 2 leaves both.  Three launches on the current stream, no host sync."""
    require_device(image, "image")
    require_device(target, "target")
    if image.dtype != torch.float32 or target.dtype != torch.float32 or image.dim() != 4 or image.shape != target.shape \
            or image.device != target.device or image.numel() == 0:
        raise RuntimeError(f"psnr_ssim: float32 [B, C, H, W] image and target of one shape on one device are needed, got "
                           f"{image.dtype} {tuple(image.shape)} and {target.dtype} {tuple(target.shape)}")
    window, mode = int(window), int(unnormalize)
    b, c, h, w = image.shape
    if window % 2 != 1 or not 3 <= window <= 11 or h <= window // 2 or w <= window // 2:
        raise RuntimeError(f"psnr_ssim: window {window} must be odd in 3..11 and H, W = {h}, {w} larger than window // 2")
    if mode not in (UNNORMALIZE_AUTO, UNNORMALIZE_ALWAYS, UNNORMALIZE_NEVER):
        raise RuntimeError(f"psnr_ssim: unnormalize {unnormalize} is not 0 (by the minimum), 1 (always) or 2 (never)")
    image, target = image.contiguous(), target.contiguous()
    psnr = torch.empty((b,), dtype=torch.float32, device=image.device)
    ssim = torch.empty((b,), dtype=torch.float32, device=image.device)
    smap = torch.empty((b, c, h, w), dtype=torch.float32, device=image.device) if return_map else None
    ws_bytes = int(lib().sis_psnr_ssim_workspace_bytes(b, c, h, w))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=image.device)
    n = image.numel()
    reads = (3.0 if mode == UNNORMALIZE_AUTO else 2.0) * 4.0 * n
    taps = 2.0 * window * 5 * 2   # row + column pass of five moments, one FMA per tap
    with torch.cuda.device(image.device):
        _check(_launch("psnr_ssim_tile_kernel", (taps + 40.0) * n, reads + (4.0 * n if return_map else 0.0),
                       lambda: lib().sis_psnr_ssim(_ptr(psnr), _ptr(ssim), _ptr(smap), _ptr(image), _ptr(target), b, c, h, w, window,
                                                   float(max_val), mode, _ptr(ws), ws_bytes, _stream())), "sis_psnr_ssim")
    return (psnr, ssim, smap) if return_map else (psnr, ssim)


def autoencoder_batch(images, ids, scale, per_channel, seed, grey):
    """Resident uint8 [N, 3, S, S], int32 ids [B] and the per-sample noise parameters (device tensors [B]: float32 ``scale``,
    int32 ``per_channel``, int32 ``seed`` -- its 32 bits are the seed word --, int32 ``grey``) -> (input_image, output_image),
    float32 [B, 3, S, S]: the reference's (Denoising / BlackAndWhiteDenoising)AutoencoderDataset batch in one launch.
    ``output_image`` equals ``gan_image_batch``; ``input_image`` is the same map of clip(rint(p + scale * z), 0, 255), grey
    after the noise where asked.  The caller keeps the ids inside 0 .. N - 1 (an id outside yields NaN samples)."""
    require_device(images, "images")
    require_device(ids, "ids")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise RuntimeError(f"autoencoder_batch: uint8 [N, 3, S, S] images are needed, got {images.dtype} {tuple(images.shape)}")
    if ids.dtype != torch.int32 or ids.dim() != 1 or ids.numel() == 0 or ids.device != images.device:
        raise RuntimeError("autoencoder_batch: int32 [B] ids on the images' device are needed")
    for t, name, dtype in ((scale, "scale", torch.float32), (per_channel, "per_channel", torch.int32), (seed, "seed", torch.int32),
                           (grey, "grey", torch.int32)):
        require_device(t, name)
        if t.dtype != dtype or tuple(t.shape) != tuple(ids.shape) or t.device != images.device:
            raise RuntimeError(f"autoencoder_batch: {name} must be a {dtype} [B] tensor on the images' device, got {t.dtype} {tuple(t.shape)}")
    images, ids = images.contiguous(), ids.contiguous()
    scale, per_channel, seed, grey = scale.contiguous(), per_channel.contiguous(), seed.contiguous(), grey.contiguous()
    n, _, size, _ = images.shape
    b = ids.numel()
    inp = torch.empty((b, 3, size, size), dtype=torch.float32, device=images.device)
    out = torch.empty((b, 3, size, size), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        _check(_launch("autoencoder_batch_kernel", 0.0, 9.0 * out.numel(),
                       lambda: lib().sis_autoencoder_batch(_ptr(inp), _ptr(out), _ptr(images), _ptr(ids), _ptr(scale), _ptr(per_channel),
                                                           _ptr(seed), _ptr(grey), n, b, size, _stream())), "sis_autoencoder_batch")
    return inp, out


# ------------------------------------------------------------------------------ dataset ground truth (csrc/coco_gt.h)

LabelRegions = collections.namedtuple("LabelRegions", "has region_count regions run_total runs")
LABEL_REGIONS_MAX_CLASSES = 8


def label_regions_capacity(p):
    """(max_regions, max_runs) of the worst cases: an aligned 2x2 block holds pixels of one region at most;
    p*p + 1 counts and one more per region."""
    regions = ((int(p) + 1) // 2) ** 2
    return regions, int(p) * int(p) + 1 + regions


def label_regions(label, colours, runs=True, max_regions=None, max_runs=None):
    """uint8 [B, p, p, 3] label images (device) and the annotated classes' colours (host, [K][3] integers) -> a ``LabelRegions``
    of device tensors: ``has`` uint8 [B, K], ``region_count`` and ``run_total`` int32 [B, K] (the true numbers),
    ``regions`` int32 [B, K, max_regions, 8] with rows (root, x0, y0, w, h, area, run_offset, run_count) in ascending root order,
    ``runs`` int32 [B, K, max_runs]: COCO's uncompressed column-major run lengths of every region that is not a straight
    stroke, region after region.  ``runs=False`` is the listing mode (``runs`` is None, the table is still complete);
    ``max_regions=0`` stores no rows (``regions`` is None).  The capacities default to what no plane can exceed.  Fixed launch
    sequence on the current stream, no host sync."""
    require_device(label, "label")
    if label.dtype != torch.uint8 or label.dim() != 4 or label.shape[3] != 3 or label.shape[1] != label.shape[2] or label.shape[0] < 1 \
            or label.shape[1] < 1:
        raise RuntimeError(f"label_regions: uint8 [B, p, p, 3] label images are needed, got {label.dtype} {tuple(label.shape)}")
    flat = [int(v) for colour in colours for v in colour]
    k = len(flat) // 3
    if k < 1 or k > LABEL_REGIONS_MAX_CLASSES or len(flat) != 3 * k or any(len(colour) != 3 for colour in colours) \
            or any(not 0 <= v <= 255 for v in flat):
        raise RuntimeError(f"label_regions: 1..{LABEL_REGIONS_MAX_CLASSES} colours of three bytes are needed, got {colours!r}")
    label = label.contiguous()
    b, p = label.shape[0], label.shape[1]
    worst_regions, worst_runs = label_regions_capacity(p)
    max_regions = worst_regions if max_regions is None else int(max_regions)
    max_runs = worst_runs if max_runs is None else int(max_runs)
    if max_regions < 0 or max_runs < 0:
        raise RuntimeError("label_regions: negative capacity")
    dev = label.device
    has = torch.empty((b, k), dtype=torch.uint8, device=dev)
    region_count = torch.empty((b, k), dtype=torch.int32, device=dev)
    run_total = torch.empty((b, k), dtype=torch.int32, device=dev)
    regions = torch.empty((b, k, max_regions, 8), dtype=torch.int32, device=dev) if max_regions > 0 else None
    counts = torch.empty((b, k, max_runs), dtype=torch.int32, device=dev) if runs else None
    ws_bytes = int(lib().sis_label_regions_workspace_bytes(b, k, p))
    ws = torch.empty(((max(ws_bytes, 4) + 3) // 4,), dtype=torch.int32, device=dev)
    c_colours = (ctypes.c_uint8 * (3 * k))(*flat)
    with torch.cuda.device(dev):
        _check(_launch("gt_stats_kernel", 0.0, 3.0 * label.numel() + 30.0 * b * k * p * p,
                       lambda: lib().sis_label_regions(_ptr(has), _ptr(region_count), _ptr(regions), _ptr(run_total), _ptr(counts),
                                                       _ptr(label), c_colours, k, b, p, max_regions, max_runs, _ptr(ws),
                                                       ws.numel() * 4, _stream())), "sis_label_regions")
    return LabelRegions(has, region_count, regions, run_total, counts)


# ------------------------------------------------------------------------------ page visualisation (csrc/page_visual.h)

PageRegions = collections.namedtuple("PageRegions", "regions region_count kept_count region_labels")
PageRender = collections.namedtuple("PageRender", "segmented overlay boxes_on_page boxes_on_segmented")
PAGE_MAX_EDGE, PAGE_MAX_CLASSES, PAGE_GRADIENT_STEPS = 8192, 16, 100
PAGE_DEFAULT_MAX_REGIONS = 4096
PAGE_RENDER_OUTPUTS = PageRender._fields


def _page_pred(pred, who):
    require_device(pred, "pred")
    if pred.dtype != torch.float32 or pred.dim() != 3:
        raise RuntimeError(f"{who}: float32 [classes, H, W] confidences are needed, got {pred.dtype} {tuple(pred.shape)}")
    return pred.contiguous()


def _page_image(page, height, width, who):
    require_device(page, "page")
    if page.dim() == 2:
        page = page.unsqueeze(-1)
    if page.dtype != torch.uint8 or page.dim() != 3 or page.shape[2] not in (1, 3) or tuple(page.shape[:2]) != (height, width):
        raise RuntimeError(f"{who}: a uint8 [{height}, {width}, 1 or 3] page is needed, got {page.dtype} {tuple(page.shape)}")
    return page.contiguous()


def page_regions_capacity(height, width):
    """The number of regions no plane can exceed: an aligned 2x2 block holds pixels of one region at most."""
    return ((int(height) + 1) // 2) * ((int(width) + 1) // 2)


def page_regions(pred, background_class_id=0, filter_classes=(), min_contour_area=10, max_regions=None, labels=True):
    """float32 [classes, H, W] confidences of an assembled page (device) -> a ``PageRegions`` of device tensors (DESIGN.md
    §17.1): ``regions`` int32 [classes, max_regions, 8] with rows (root, x0, y0, w, h, twice_area, kept, 0) in ascending root
    order, ``region_count`` and ``kept_count`` int32 [classes] (the true numbers, also above ``max_regions``), ``region_labels``
    int32 [classes, H, W] (root + 1 per pixel, 0 outside any region; None with ``labels=False``).  The background plane and the
    planes in ``filter_classes`` are skipped: zero counts, zero labels.  Rows from the count on are not written.
    ``max_regions`` defaults to ``min(page_regions_capacity(H, W), PAGE_DEFAULT_MAX_REGIONS)``; 0 stores no rows (``regions``
    is None).  Fixed launch sequence on the current stream, no host sync."""
    pred = _page_pred(pred, "page_regions")
    classes, height, width = pred.shape
    mask = 0
    for k in filter_classes:
        if not 0 <= int(k) < classes:
            raise RuntimeError(f"page_regions: filter class {k} outside the {classes} classes")
        mask |= 1 << int(k)
    if max_regions is None:
        max_regions = min(page_regions_capacity(height, width), PAGE_DEFAULT_MAX_REGIONS)
    max_regions = int(max_regions)
    if max_regions < 0:
        raise RuntimeError("page_regions: negative capacity")
    dev = pred.device
    regions = torch.empty((classes, max_regions, 8), dtype=torch.int32, device=dev) if max_regions > 0 else None
    region_count = torch.empty((classes,), dtype=torch.int32, device=dev)
    kept_count = torch.empty((classes,), dtype=torch.int32, device=dev)
    region_labels = torch.empty((classes, height, width), dtype=torch.int32, device=dev) if labels else None
    ws_bytes = int(lib().sis_page_regions_workspace_bytes(classes, height, width))
    ws = torch.empty(((max(ws_bytes, 4) + 3) // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("pv_box_kernel", 0.0, 40.0 * pred.numel(),
                       lambda: lib().sis_page_regions(_ptr(regions), _ptr(region_count), _ptr(kept_count), _ptr(region_labels),
                                                      _ptr(pred), classes, height, width, int(background_class_id), mask,
                                                      int(min_contour_area), max_regions, _ptr(ws), ws.numel() * 4, _stream())),
               "sis_page_regions")
    return PageRegions(regions, region_count, kept_count, region_labels)


def page_confidence_table(colours):
    """[classes][100][3] integers: per class the reference's ``linear_gradient((255, 255, 255), colour, 100)``
    (visualization/utils.py:9-26), entry t = int(255 + (t / 99) * (c - 255)) in Python float arithmetic, entry 0 white."""
    n = PAGE_GRADIENT_STEPS
    return [[[255, 255, 255]] + [[int(255 + (float(t) / (n - 1)) * (int(c) - 255)) for c in colour] for t in range(1, n)]
            for colour in colours]


def _page_colours(colours, classes, who):
    flat = [int(v) for colour in colours for v in colour]
    if len(flat) != 3 * classes or any(len(colour) != 3 for colour in colours) or any(not 0 <= v <= 255 for v in flat):
        raise RuntimeError(f"{who}: {classes} colours of three bytes are needed, got {colours!r}")
    return flat


def page_render(pred, page, colours, background_class_id=0, confidence_table=None, regions=None, region_count=None,
                patch_boxes=None, outputs=PAGE_RENDER_OUTPUTS):
    """The page's pictures as a ``PageRender`` of uint8 [H, W, 3] device tensors, None for every name not in
    ``outputs``.  ``pred`` float32 [classes, H, W]; ``page`` uint8 [H, W, 1 or 3] (may be None when neither ``overlay`` nor
    ``boxes_on_page`` is asked for); ``colours`` [classes][3] host integers; ``confidence_table`` uint8 [classes, 100, 3] on the
    device (``page_confidence_table`` uploaded) selects the confidence mode; ``regions`` / ``region_count`` are
    ``page_regions``' tables, whose kept rows are outlined in green, stroke 3; ``patch_boxes`` int32 [m, 4] on the device
    (x0, y0, x1, y1, inclusive) are outlined in red, stroke 1, afterwards.  At most three launches on the current stream."""
    pred = _page_pred(pred, "page_render")
    classes, height, width = pred.shape
    unknown = [name for name in outputs if name not in PAGE_RENDER_OUTPUTS]
    if unknown or not outputs:
        raise RuntimeError(f"page_render: outputs must be some of {PAGE_RENDER_OUTPUTS}, got {tuple(outputs)}")
    flat = _page_colours(colours, classes, "page_render")
    if page is not None:
        page = _page_image(page, height, width, "page_render")
    elif "overlay" in outputs or "boxes_on_page" in outputs:
        raise RuntimeError("page_render: overlay and boxes_on_page need the page")
    dev = pred.device
    if confidence_table is not None:
        require_device(confidence_table, "confidence_table")
        if confidence_table.dtype != torch.uint8 or tuple(confidence_table.shape) != (classes, PAGE_GRADIENT_STEPS, 3):
            raise RuntimeError(f"page_render: a uint8 [{classes}, {PAGE_GRADIENT_STEPS}, 3] confidence table is needed")
        confidence_table = confidence_table.contiguous()
    max_regions = 0
    if regions is not None:
        require_device(regions, "regions")
        if regions.dtype != torch.int32 or regions.dim() != 3 or regions.shape[0] != classes or regions.shape[2] != 8 \
                or region_count is None or region_count.dtype != torch.int32 or tuple(region_count.shape) != (classes,) \
                or not region_count.is_cuda:
            raise RuntimeError("page_render: regions int32 [classes, max_regions, 8] and region_count int32 [classes] are needed")
        regions, region_count, max_regions = regions.contiguous(), region_count.contiguous(), regions.shape[1]
    patches = 0
    if patch_boxes is not None:
        require_device(patch_boxes, "patch_boxes")
        if patch_boxes.dtype != torch.int32 or patch_boxes.dim() != 2 or patch_boxes.shape[1] != 4:
            raise RuntimeError("page_render: int32 [m, 4] patch boxes are needed")
        patch_boxes, patches = patch_boxes.contiguous(), patch_boxes.shape[0]
    images = [torch.empty((height, width, 3), dtype=torch.uint8, device=dev) if name in outputs else None
              for name in PAGE_RENDER_OUTPUTS]
    c_colours = (ctypes.c_uint8 * (3 * classes))(*flat)
    with torch.cuda.device(dev):
        _check(_launch("pv_colour_kernel", 0.0, 4.0 * pred.numel() + 3.0 * height * width * (1 + len(outputs)),
                       lambda: lib().sis_page_render(*[_ptr(t) for t in images], _ptr(pred), _ptr(page),
                                                     0 if page is None else page.shape[2], c_colours, _ptr(confidence_table),
                                                     _ptr(regions) if max_regions else None,
                                                     _ptr(region_count) if max_regions else None, max_regions,
                                                     _ptr(patch_boxes) if patches else None, patches, classes, height, width,
                                                     int(background_class_id), _stream())), "sis_page_render")
    return PageRender(*images)


def page_crops(page, rows, mode, region_labels=None):
    """Cut-out regions of a page.  ``rows``: host sequence or array of (plane, root, x0, y0, w, h); ``mode`` "bbox"
    copies the page's pixels, "contour" keeps them where ``region_labels`` (``page_regions``' int32 [classes, H, W]) equals
    root + 1 and paints (255, 255, 255) elsewhere.  Returns (packed uint8 device buffer, list of byte offsets): crop i is
    ``buffer[offsets[i]:offsets[i] + h * w * 3].view(h, w, 3)``.  One table upload, one launch on the current stream."""
    if mode not in ("bbox", "contour"):
        raise RuntimeError(f"page_crops: mode must be 'bbox' or 'contour', got {mode!r}")
    require_device(page, "page")
    if page.dim() == 2:
        page = page.unsqueeze(-1)
    height, width = int(page.shape[0]), int(page.shape[1])
    page = _page_image(page, height, width, "page_crops")
    classes = PAGE_MAX_CLASSES
    if mode == "contour":
        if region_labels is None or not region_labels.is_cuda or region_labels.dtype != torch.int32 or region_labels.dim() != 3 \
                or tuple(region_labels.shape[1:]) != (height, width):
            raise RuntimeError(f"page_crops: contour mode needs int32 [classes, {height}, {width}] region labels on the device")
        region_labels, classes = region_labels.contiguous(), region_labels.shape[0]
    else:
        region_labels = None
    table = torch.as_tensor(rows, dtype=torch.int64).reshape(-1, 6)   # on the host: plane, root, x0, y0, w, h
    plane, x0, y0, w, h = table[:, 0], table[:, 2], table[:, 3], table[:, 4], table[:, 5]
    bad = (plane < 0) | (plane >= classes) | (x0 < 0) | (y0 < 0) | (w < 1) | (h < 1) | (x0 + w > width) | (y0 + h > height)
    if bool(bad.any()):
        row = tuple(table[int(bad.nonzero()[0])].tolist())
        raise RuntimeError(f"page_crops: row {row} leaves the {height} x {width} page")
    sizes = 3 * w * h
    ends = torch.cumsum(sizes, 0)
    total = int(ends[-1]) if len(table) else 0
    offsets = (ends - sizes).tolist()
    dev = page.device
    out = torch.empty((total,), dtype=torch.uint8, device=dev)
    if not len(table):
        return out, offsets
    device_table = torch.empty((len(table), 7), dtype=torch.int64, device=dev)
    device_table.copy_(torch.cat([table, (ends - sizes)[:, None]], dim=1))
    with torch.cuda.device(dev):
        _check(_launch("pv_crops_kernel", 0.0, 2.0 * total,
                       lambda: lib().sis_page_crops(_ptr(out), total, _ptr(device_table), len(table), _ptr(page), page.shape[2],
                                                    _ptr(region_labels), classes, height, width, 1 if mode == "contour" else 0,
                                                    _stream())), "sis_page_crops")
    return out, offsets


# ------------------------------------------------------------------------------ scan patches (csrc/scan_patches.h)


def _scan_page(page, what):
    require_device(page, "page")
    if page.dtype != torch.uint8 or page.dim() != 3 or page.shape[2] != 3 or page.shape[0] < 1 or page.shape[1] < 1:
        raise RuntimeError(f"{what}: a uint8 [H, W, 3] page is needed, got {page.dtype} {tuple(page.shape)}")
    return page.contiguous()


def scan_reduce(page, fx, fy):
    """uint8 [H, W, 3] page (device) -> uint8 [ceil(H / fy), ceil(W / fx), 3]: Pillow's ``Image.reduce((fx, fy))``, byte for
    byte; ragged last rows and columns are averaged over the pixels that exist.  One launch on the current stream."""
    page = _scan_page(page, "scan_reduce")
    h, w = int(page.shape[0]), int(page.shape[1])
    fx, fy = int(fx), int(fy)
    if fx < 1 or fy < 1:
        raise RuntimeError(f"scan_reduce: factors ({fx}, {fy}) must be >= 1")
    out = torch.empty((-(-h // fy), -(-w // fx), 3), dtype=torch.uint8, device=page.device)
    with torch.cuda.device(page.device):
        _check(_launch("scan_reduce_kernel", 0.0, float(page.numel() + out.numel()),
                       lambda: lib().sis_scan_reduce(_ptr(out), _ptr(page), h, w, fx, fy, _stream())), "sis_scan_reduce")
    return out


def _scan_axis_tables(table, in_size, out_size, device, what):
    """One axis' host table (utils.scan_patches.AxisTable) checked and uploaded: (coef, first, count, ksize)."""
    if table is None:
        return None, None, None, 0
    coef = torch.tensor(table.coef, dtype=torch.int32).reshape(out_size, table.ksize)
    first = torch.tensor(table.first, dtype=torch.int32).reshape(out_size)
    count = torch.tensor(table.count, dtype=torch.int32).reshape(out_size)
    if bool((first < 0).any()) or bool((count < 0).any()) or bool((count > table.ksize).any()) or bool((first + count > in_size).any()):
        raise RuntimeError(f"{what}: a tap of the table leaves the {in_size} source pixels")
    on_device = []
    for host in (coef, first, count):
        t = torch.empty(host.shape, dtype=torch.int32, device=device)
        t.copy_(host)
        on_device.append(t)
    return on_device[0], on_device[1], on_device[2], int(table.ksize)


def scan_resample_plan(page, plan):
    """One two-pass antialiased resample of a uint8 [H, W, 3] page (device) from the host tables of ``plan``
    (utils.scan_patches.ResamplePlan: output size, horizontal and vertical AxisTable, None for a pass Pillow skips) ->
    uint8 [h, w, 3].  Horizontal pass first, its uint8 result in a workspace; at most two launches on the current stream."""
    page = _scan_page(page, "scan_resample")
    h, w = int(page.shape[0]), int(page.shape[1])
    out_w, out_h = (int(v) for v in plan.size)
    dev = page.device
    cx, fx, nx, kx = _scan_axis_tables(plan.horizontal, w, out_w, dev, "scan_resample")
    cy, fy, ny, ky = _scan_axis_tables(plan.vertical, h, out_h, dev, "scan_resample")
    out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=dev)
    ws, ws_bytes = None, 0
    if kx and ky:
        ws_bytes = int(lib().sis_scan_resample_workspace_bytes(h, w, out_h, out_w))
        ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("scan_hpass_kernel", 0.0, float(page.numel() + 2 * ws_bytes + out.numel()),
                       lambda: lib().sis_scan_resample(_ptr(out), _ptr(page), h, w, out_h, out_w, _ptr(cx), _ptr(fx), _ptr(nx), kx, _ptr(cy),
                                                       _ptr(fy), _ptr(ny), ky, _ptr(ws), ws_bytes, _stream())), "sis_scan_resample")
    return out


def scan_resample(page, size, box=None):
    """uint8 [H, W, 3] page (device) -> uint8 [h, w, 3] for ``size`` = (w, h): Pillow's ``Image.resize(size, BICUBIC, box=box,
    reducing_gap=None)``, byte for byte.  The taps are built on the host (utils/scan_patches.py)."""
    from utils import scan_patches as tables
    page = _scan_page(page, "scan_resample")
    for plan in tables.resize_plans(int(page.shape[1]), int(page.shape[0]), (int(size[0]), int(size[1])), box):
        page = scan_resample_plan(page, plan)
    return page


def scan_thumbnail(page, size):
    """uint8 [H, W, 3] page (device) -> what ``Image.thumbnail((size, size))`` leaves of a fully decoded RGB image, byte for
    byte: BICUBIC, reducing_gap 2.0 (``scan_reduce`` by ``int(W / w / 2) or 1`` per axis, then ``scan_resample`` from the box
    (0, 0, W / fx, H / fy)).  A page that already fits is returned as it is, the same tensor."""
    from utils import scan_patches as tables
    page = _scan_page(page, "scan_thumbnail")
    plan = tables.thumbnail_plan(int(page.shape[1]), int(page.shape[0]), size)
    if plan is None:
        return page
    if plan.factors != (1, 1):
        page = scan_reduce(page, *plan.factors)
    for step in plan.resamples:
        page = scan_resample_plan(page, step)
    return page


def scan_patches(page, origins, size):
    """``size`` x ``size`` windows of a uint8 [H, W, 3] page (device) at ``origins`` -- a host sequence of (x, y) or an int32
    [n, 2] device tensor -- gathered into uint8 [n, size, size, 3], 0 outside the page (``Image.crop``'s black).  The result
    is what ``png_encode_pairs`` takes as its images.  One table upload, one launch on the current stream."""
    page = _scan_page(page, "scan_patches")
    h, w = int(page.shape[0]), int(page.shape[1])
    size = int(size)
    dev = page.device
    if isinstance(origins, torch.Tensor) and origins.is_cuda:
        if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.device != dev:
            raise RuntimeError(f"scan_patches: device origins must be int32 [n, 2] on the page's device, got {origins.dtype} "
                               f"{tuple(origins.shape)}")
        table = origins.contiguous()
    else:
        host = torch.as_tensor(origins, dtype=torch.int32).reshape(-1, 2)
        table = torch.empty(host.shape, dtype=torch.int32, device=dev)
        table.copy_(host)
    n = int(table.shape[0])
    if n < 1 or size < 1:
        raise RuntimeError(f"scan_patches: {n} windows of size {size}: both must be >= 1")
    out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("scan_patches_kernel", 0.0, 2.0 * out.numel(),
                       lambda: lib().sis_scan_patches(_ptr(out), _ptr(page), _ptr(table), n, size, h, w, _stream())), "sis_scan_patches")
    return out


# ------------------------------------------------------------------------------ scanner margin (csrc/scan_margin.h)
SCAN_MARGIN_MIN_SIDE, SCAN_MARGIN_MAX_SIDE = 3, 4096
ScanContentBox = collections.namedtuple("ScanContentBox", "box info edges contours")


def scan_content_box(page, low=20, high=150, edges=False, max_contours=0):
    """uint8 [h, w, 3] analysis image (device, 3 <= h, w <= 4096) -> a ``ScanContentBox`` of device tensors (the
    reference's ``get_content_box`` with ``edge_detect=True``): ``box`` int32 [4] = x0, y0, x1, y1 with exclusive ends, ``info``
    int32 [8] = contours, outer contours, largest box area, contours kept, decision (0 cut at the largest gap of the box areas,
    1 at most one contour, 2 largest area below 0.6 of the image: the last two give the whole image), T, pixels of E, 0;
    ``edges`` uint8 [h, w] = the closed edge image E as 0 / 255 (None unless asked for); ``contours`` int32 [max_contours, 6] =
    kind (0 outer, 1 hole), root, x0, y0, w, h in the order outers by root, then holes by root (None for 0), rows from
    ``info[0]`` on not written.  Fixed launch sequence on the current stream, no host sync."""
    page = _scan_page(page, "scan_content_box")
    h, w = int(page.shape[0]), int(page.shape[1])
    max_contours = int(max_contours)
    if not (SCAN_MARGIN_MIN_SIDE <= h <= SCAN_MARGIN_MAX_SIDE and SCAN_MARGIN_MIN_SIDE <= w <= SCAN_MARGIN_MAX_SIDE):
        raise RuntimeError(f"scan_content_box: image {h} x {w} outside {SCAN_MARGIN_MIN_SIDE}..{SCAN_MARGIN_MAX_SIDE} a side")
    if max_contours < 0:
        raise RuntimeError("scan_content_box: negative max_contours")
    dev = page.device
    box = torch.empty((4,), dtype=torch.int32, device=dev)
    info = torch.empty((8,), dtype=torch.int32, device=dev)
    edge_image = torch.empty((h, w), dtype=torch.uint8, device=dev) if edges else None
    table = torch.empty((max_contours, 6), dtype=torch.int32, device=dev) if max_contours > 0 else None
    ws_bytes = int(lib().sis_scan_content_box_workspace_bytes(h, w))
    ws = torch.empty(((max(ws_bytes, 4) + 3) // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_launch("margin_front_kernel", 0.0, 60.0 * h * w,
                       lambda: lib().sis_scan_content_box(_ptr(box), _ptr(info), _ptr(edge_image), _ptr(table), max_contours, _ptr(page),
                                                          h, w, int(low), int(high), _ptr(ws), ws.numel() * 4, _stream())),
               "sis_scan_content_box")
    return ScanContentBox(box, info, edge_image, table)


def scan_remove_margin(page, analysis_size=1000):
    """uint8 [H, W, 3] page (device) -> (cropped page, box, crop): the reference's ``remove_scanning_margin``.  ``box`` is the
    content box of ``scan_thumbnail(page, analysis_size)`` (``scan_content_box``), ``crop`` that box scaled to the page
    (``utils.scan_patches.scale_bounding_box``), both Python lists [x0, y0, x1, y1]; the cropped page is contiguous.
    ONE host read, of ``box``: the sizes of the thumbnails that follow are decided on the host from the size of the cropped
    page, so the crop has to be known there."""
    from utils import scan_patches as tables
    page = _scan_page(page, "scan_remove_margin")
    analysis = scan_thumbnail(page, analysis_size)
    box = [int(v) for v in scan_content_box(analysis).box.tolist()]   # the one host read
    crop = tables.scale_bounding_box(box, (int(analysis.shape[1]), int(analysis.shape[0])), (int(page.shape[1]), int(page.shape[0])))
    window = page[crop[1]:crop[3], crop[0]:crop[2]]
    cropped = torch.empty(tuple(window.shape), dtype=torch.uint8, device=page.device)
    cropped.copy_(window)
    return cropped, box, crop
