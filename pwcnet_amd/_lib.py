"""ctypes binding of libpwc_hip.so (the C ABI declared in include/pwc_hip.h).

The library is the ONLY compute path of this package: if it is missing or does not
export every declared symbol, importing the ops fails loudly -- there is no CPU or
eager-PyTorch fallback.  torch must be imported first so that the HIP runtime the
library binds to (libamdhip64.so.7) is the one PyTorch already loaded.
"""
import ctypes
import os
import subprocess

import torch  # noqa: F401  (loads libamdhip64 before libpwc_hip.so)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# PWC_HARNESS=1 (the A/B scripts under scripts/ set it before importing this package; nothing else does): load
# libpwc_hip_harness.so instead -- the same sources compiled with -DPWC_HARNESS, which adds the process-wide pwc_debug_* knobs
# (tile pinning, ablations).  The production library exports none of them (tests/test_host.py checks).
HARNESS = os.environ.get("PWC_HARNESS", "") == "1"
LIB_PATH = os.path.join(CSRC, "libpwc_hip_harness.so" if HARNESS else "libpwc_hip.so")
HARNESS_SIGNATURES_NAMES = ("pwc_debug_cost_volume_blk_rows", "pwc_debug_conv3x3_sk_tile", "pwc_debug_conv3x3_t32",
                            "pwc_debug_h2_reserve_cus", "pwc_debug_conv3x3_s2_tile")
SOURCES = ["conv3x3_mfma.hip", "conv3x3_wino.hip", "conv3x3_direct.hip", "cost_volume.hip", "pwc_ops.hip",
           "pwc_backward.hip", "conv3x3_wgrad.hip", "conv3x3_h2.hip", "conv3x3_c16pair.hip", "conv3x3_sk.hip", "conv3x3_s2.hip", "conv3x3_t32.hip", "conv3x3_w32.hip",
           "pwc_flow_loss.hip", "pwc_unsup.hip", "pwc_census.hip", "pwc_ssim.hip", "pwc_fbcheck.hip", "pwc_fit.hip", "pwc_augment.hip", "pwc_splat.hip", "pwc_pyramid.hip", "pwc_featnorm.hip", "pwc_distill.hip", "pwc_compose.hip", "pwc_flowvis.hip", "pwc_track.hip", "pwc_interp.hip", "pwc_motion.hip", "pwc_regions.hip", "pwc_region_links.hip", "pwc_flow_filter.hip", "pwc_temporal.hip", "pwc_plate.hip", "pwc_homography.hip", "pwc_fundamental.hip", "pwc_pose.hip", "pwc_trajectory.hip", "pwc_pose_refine.hip"]
HEADERS = ["pwc_common.h", "conv_fp32_common.h", "cost_volume_common.h", "loss_common.h", "motion_ldlt.h", "motion_jacobi.h", "two_view.h", "projective.h", "flow_record.h", "robust_fit.h", "cost_volume_roll.hip", "cost_volume_mfma.hip", "cost_volume_h2.hip", "cost_volume_blk.hip", "conv3x3_wino4.hip", os.path.join("..", "..", "include", "pwc_hip.h")]

_vp, _i, _f, _l, _sz, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); mirrors include/pwc_hip.h one to one
SIGNATURES = {
    "pwc_version": (_i, []),
    "pwc_error_string": (ctypes.c_char_p, [_i]),
    "pwc_cost_volume_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_cost_volume_uses_rolling_kernel": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "pwc_warp_bilinear_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _vp]),
    "pwc_warp_nearest_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _vp]),
    "pwc_cost_volume_coarse_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_resize_bilinear_pair_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_warp_copy_f32": (_i, [_i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
    "pwc_warp_cost_volume_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_warp_cost_volume_concat_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_warp_cost_volume_concat_h2_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_warp_cost_volume_concat_blk_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_warp_cost_volume_concat_supported": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "pwc_warp_cost_volume_concat_blk_supported": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp]),
    "pwc_conv3x3_workspace_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_plan": (_i, [_i, _i, _i, ctypes.POINTER(_i)]),
    "pwc_conv3x3_uses_halo_kernel": (_i, [_i, _i, _i, _i, _i]),
    "pwc_conv3x3_tile_shape": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "pwc_conv3x3_wino_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_wino_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_wino_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_wino_workgroups": (_l, [_i, _i, _i, _i, _i]),
    "pwc_conv3x3_wino4_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_wino4_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_wino4_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_wino4_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_h2_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_h2_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_h2_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "pwc_conv3x3_h2_ex_f32": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp, _vp]),
    "pwc_conv3x3_h2_ex3_f32": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp, _vp]),
    "pwc_conv3x3_h2_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_h2_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_h2_plan": (_i, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_h2_stride2_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp, _vp]),
    "pwc_conv3x3_h2_stride2_supported": (_i, [_i, _i, _i, _i, _i]),
    "pwc_conv3x3_sk_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_sk_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_sk_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_sk_supported": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_sk_variant_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "pwc_conv3x3_t32_packed_floats": (_sz, [_i]),
    "pwc_conv3x3_t32_pack_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pwc_conv3x3_t32_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_t32_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_w32_packed_floats": (_sz, [_i]),
    "pwc_conv3x3_w32_pack_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pwc_conv3x3_w32_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_w32_supported": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_h2_stride2_packed_floats": (_sz, [_i, _i]),
    "pwc_conv3x3_h2_stride2_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pwc_conv3x3_h2_stride2_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "pwc_conv3x3_c16pair_packed_floats": (_sz, []),
    "pwc_conv3x3_c16pair_pack_f32": (_i, [_vp, _vp, _vp, _vp]),
    "pwc_conv3x3_c16pair_f32": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_c16pair_supported": (_i, [_i, _i, _i]),
    "pwc_conv3x3_c3c16pair_packed_floats": (_sz, []),
    "pwc_conv3x3_c3c16pair_pack_f32": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "pwc_conv3x3_c3c16pair_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pwc_conv3x3_c3c16pair_supported": (_i, [_i, _i, _i]),
    "pwc_conv3x3_h2_variant_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "pwc_conv3x3_wino_split_plan": (_i, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_wino_split_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "pwc_conv3x3_wino_split_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "pwc_conv3x3_direct_f32": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_resize_bilinear_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_resize_bilinear_status_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "pwc_absmax_f32": (_i, [_vp, _i, _l, _i, _vp, _vp]),
    "pwc_copy_channels_f32": (_i, [_vp, _i, _vp, _i, _l, _i, _vp]),
    "pwc_device_spin": (_i, [ctypes.c_longlong, _vp]),
    "pwc_device_touch": (_i, [_vp, _vp]),
    "pwc_lrelu_grad_f32": (_i, [_vp, _i, _vp, _i, _l, _i, _f, _vp]),
    "pwc_add_f32": (_i, [_vp, _i, _vp, _i, _l, _i, _f, _i, _vp]),
    "pwc_channel_sums_workspace_floats": (_sz, [_l, _i]),
    "pwc_channel_sums_f32": (_i, [_vp, _i, _l, _i, _vp, _sz, _vp, _i, _vp]),
    "pwc_lrelu_grad_channel_sums_f32": (_i, [_vp, _i, _vp, _i, _l, _i, _f, _vp, _sz, _vp, _i, _vp]),
    "pwc_resize_bilinear_grad_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "pwc_warp_bilinear_grad_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_warp_bilinear_grad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_warp_bilinear_grad_det_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "pwc_cost_volume_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "pwc_flow_norm_grad_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _f, _vp, _i, _i, _vp]),
    "pwc_adam_step_f32": (_i, [_vp, _vp, _vp, _vp, _l, _f, _f, _f, _f, _f, _f, _vp]),
    "pwc_conv3x3_wgrad_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "pwc_conv3x3_wgrad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "pwc_flow_norm_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_flow_norm_sums_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp, _vp]),
    "pwc_conv3x3_dgrad_s2_narrow_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_flow_norm_masked_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_flow_norm_masked_sums_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp, _vp, _vp]),
    "pwc_flow_norm_masked_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _i, _f, _vp, _i, _i, _vp]),
    "pwc_flow_metrics_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_flow_metrics_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "pwc_photometric_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_photometric_sums_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "pwc_photometric_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _i, _i, _vp]),
    "pwc_flow_smoothness_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_flow_smoothness_sums_f32": (_i, [_vp, _i, _vp, _i, _i, _f, _f, _f, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "pwc_flow_smoothness_grad_f32": (_i, [_vp, _i, _vp, _i, _i, _f, _f, _f, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "pwc_flow_smoothness2_sums_f32": (_i, [_vp, _i, _vp, _i, _i, _f, _f, _f, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "pwc_flow_smoothness2_grad_f32": (_i, [_vp, _i, _vp, _i, _i, _f, _f, _f, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "pwc_census_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "pwc_census_sums_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "pwc_census_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _vp, _sz, _vp, _i, _i, _vp]),
    "pwc_ssim_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "pwc_ssim_sums_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "pwc_ssim_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _sz, _vp, _i, _i, _vp]),
    "pwc_fb_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_fb_valid_u8": (_i, [_vp, _i, _vp, _i, _f, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pwc_fb_consistency_workspace_floats": (_sz, [_i, _i, _i]),
    "pwc_fb_consistency_sums_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _vp, _i, _i, _i, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "pwc_fb_consistency_grad_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_fb_consistency_grad_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _vp, _i, _vp, _i, _i, _vp]),
    "pwc_splat_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_splat_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp, _vp]),
    "pwc_splat_grad_f32": (_i, [_vp, _i, _vp, _i, _f, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "pwc_fit_frames_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_refit_flow_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_augment_pairs_f32": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pwc_frame_pyramid_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "pwc_mask_pyramid_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "pwc_feature_norm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_feature_norm_parts": (_i, [_i, _i, _i]),
    "pwc_feature_norm_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _d, _vp, _sz, _vp, _i, _vp, _i, _vp, _vp]),
    "pwc_feature_norm_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp, _i, _i, _vp]),
    "pwc_flow_distill_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_flow_distill_sums_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _d, _d, _vp, _vp, _vp, _sz, _vp]),
    "pwc_flow_distill_grad_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _d, _d, _vp, _vp, _i, _i, _vp]),
    "pwc_flow_compose_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "pwc_flow_compose_grad_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_flow_compose_grad_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp, _i, _vp, _i, _i, _vp]),
    "pwc_flow_max_radius_f64": (_i, [_vp, _i, _vp, _i, _i, _i, _f, _vp, _vp]),
    "pwc_flow_vis_tiles_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "pwc_flow_vis_wheel_u8": (_i, [_vp]),
    "pwc_track_points_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _f, _i, _vp, _vp, _vp]),
    "pwc_interp_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_interp_frames": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.POINTER(_d), _i, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "pwc_motion_fit_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_motion_fit_f64": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "pwc_motion_residual_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp]),
    "pwc_warp_affine": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pwc_regions_tile_h": (_i, []),
    "pwc_regions_tile_w": (_i, []),
    "pwc_regions_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_label_regions": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pwc_region_links_workspace_bytes": (_sz, [_i, _i]),
    "pwc_link_regions": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pwc_region_identities": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pwc_relabel_regions": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pwc_flow_filter_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_flow_filter_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp, _vp]),
    "pwc_temporal_filter": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _d, _d, _i, _f, _f, _i, _i, _vp, _vp, _vp]),
    "pwc_plate_build": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pwc_plate_difference": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "pwc_homography_fit_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_homography_fit_f64": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "pwc_motion_residual_projective_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp]),
    "pwc_warp_projective": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pwc_plate_build_projective": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pwc_plate_difference_projective": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "pwc_fundamental_fit_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_fundamental_fit_f64": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pwc_epipolar_residual_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp]),
    "pwc_camera_pose_workspace_bytes": (_sz, [_i]),
    "pwc_camera_pose_f64": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pwc_triangulate_depth_f32": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "pwc_scale_links_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pwc_scale_links_f32": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "pwc_camera_trajectory_f64": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pwc_pose_refine_workspace_bytes": (_sz, [_i, _i, _i]),
    "pwc_pose_refine_f64": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

if HARNESS:
    for _n in HARNESS_SIGNATURES_NAMES:
        SIGNATURES[_n] = (_i, [_i])

# status word bits of the F16-matrix-pipe kernels (include/pwc_hip.h)
STATUS_NONFINITE = 1
STATUS_STREAMK_TIMEOUT = 2
# tiles of pwc_flow_vis_tiles_u8 (include/pwc_hip.h)
VIS_FLOW, VIS_FRAME_U8, VIS_FRAME_F32, VIS_ERROR = 0, 1, 2, 3
VIS_MAX_TILES = 8
# status codes and directions of pwc_track_points_f32 (include/pwc_hip.h)
TRACK_UNSEEN, TRACK_VISIBLE, TRACK_LEFT, TRACK_OCCLUDED, TRACK_UNKNOWN = 0, 1, 2, 3, 4
TRACK_FORWARD, TRACK_BOTH = 0, 1
# frame dtypes and the longest time table of pwc_interp_frames (include/pwc_hip.h)
INTERP_U8, INTERP_F32 = 0, 1
INTERP_MAX_TIMES = 16
# models, frame dtypes and the most reweighting passes of the dominant-motion entry points (include/pwc_hip.h)
MOTION_TRANSLATION, MOTION_SIMILARITY, MOTION_AFFINE = 0, 1, 2
MOTION_U8, MOTION_F32 = 0, 1
MOTION_MAX_ITERS = 64
# the most table rows, images and pixels per image of pwc_label_regions (include/pwc_hip.h)
REGIONS_MAX_REGIONS = 65535
REGIONS_MAX_IMAGES = 65535
REGIONS_MAX_PIXELS = 1 << 26
# the most table rows of the region-tracking entry points (include/pwc_hip.h)
LINKS_MAX_REGIONS = 1024
# guide dtypes and the largest radius of pwc_flow_filter_f32 (include/pwc_hip.h)
FLOW_FILTER_U8, FLOW_FILTER_F32 = 0, 1
FLOW_FILTER_MAX_RADIUS = 7
# frame dtypes, the largest radius and the largest patch radius of pwc_temporal_filter (include/pwc_hip.h)
TEMPORAL_U8, TEMPORAL_F32 = 0, 1
TEMPORAL_MAX_RADIUS = 8
TEMPORAL_MAX_PATCH = 2
# modes and the most frames of pwc_plate_build (include/pwc_hip.h); the frame dtypes are MOTION_U8 / MOTION_F32
PLATE_MEDIAN, PLATE_MEAN = 0, 1
PLATE_MAX_FRAMES = 64
# the most pixels per image and pairs of pwc_scale_links_f32 (include/pwc_hip.h)
TRAJECTORY_MAX_PIXELS = 1 << 26
TRAJECTORY_MAX_PAIRS = 65535


class VisTile(ctypes.Structure):
    """pwc_vis_tile of include/pwc_hip.h, field for field."""
    _fields_ = [("src", _vp), ("gt", _vp), ("valid", _vp), ("max_rad", _vp), ("kind", _i), ("src_cs", _i), ("gt_cs", _i),
                ("src_h", _i), ("src_w", _i), ("x0", _i), ("tile_w", _i), ("flow_scale", _f)]


# modes of pwc_fit_frames_f32 / pwc_refit_flow_f32 (include/pwc_hip.h)
FIT_RESIZE = 0
FIT_PAD = 1

_lib = None


class PwcHipError(RuntimeError):
    pass


def _includes(path, seen=None):
    """The quoted #include closure of a source (per-object staleness check)."""
    import re
    seen = set() if seen is None else seen
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    with open(path, "r", errors="replace") as f:
        for inc in re.findall(r'^\s*#include\s+"([^"]+)"', f.read(), flags=re.M):
            _includes(os.path.normpath(os.path.join(os.path.dirname(path), inc)), seen)
    return seen


def build_library(force=False, verbose=False):
    """hipcc-compile the HIP sources for gfx950 into csrc/libpwc_hip.so (in-tree): one object per source, compiled in
    parallel and only when the source or something it includes is newer, then one link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(CSRC, "build_harness" if HARNESS else "build")
    os.makedirs(objdir, exist_ok=True)
    # -fno-slp-vectorize: hipcc otherwise packs the scalar fp32 FMA chains of the
    # correlation kernel into v_pk_fma_f32 pairs (hundreds of v_mov shuffles, VGPR spills)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-Wno-pass-failed"]
    if HARNESS:
        flags.append("-DPWC_HARNESS")
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        newest = max(os.path.getmtime(d) for d in _includes(src))
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            jobs.append([hipcc, *flags, "-c", src, "-o", obj])
    if not jobs and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(o) for o in objs):
        return LIB_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1) or 1) as pool:
        list(pool.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB_PATH])
    return LIB_PATH


def lib():
    """The loaded library; raises if it is absent (never falls back to another path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PwcHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). pwcnet_amd has no fallback compute path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise PwcHipError(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().pwc_error_string(rc).decode()
        raise PwcHipError(f"{what or 'pwc call'} failed: {msg} (code {rc})")


def current_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
