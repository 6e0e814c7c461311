"""ctypes binding of libtem_hip.so (C-ABI declared in include/tem_hip.h).

The reference has no native code; this is the binding a torch-em maintainer would add
(see INTEGRATION.md).  The product path has NO CPU fallback: if the shared library is
missing, every op raises.  `build()` compiles it in-tree with hipcc for gfx950.
"""
import ctypes
import threading
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# TEM_LIB: developer override for A/B builds of the same C-ABI (scripts/ab_lib.sh); the product path is the in-tree file
LIB_PATH = os.environ.get("TEM_LIB") or os.path.join(_HERE, "lib", "libtem_hip.so")
CSRC = os.path.join(_HERE, "csrc")

c_f32p = ctypes.c_void_p
c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_float = ctypes.c_float
c_double = ctypes.c_double
c_vp = ctypes.c_void_p
c_u32 = ctypes.c_uint32
c_u64 = ctypes.c_uint64

# name -> (restype, argtypes); must list every symbol of include/tem_hip.h
SIGNATURES = {
    "tem_last_error": (ctypes.c_char_p, []),
    "tem_version": (c_int, []),
    "tem_device_cus": (c_int, []),
    "tem_set_option": (c_int, [ctypes.c_char_p, c_i64]),
    "tem_get_option": (c_int, [ctypes.c_char_p, ctypes.POINTER(c_i64)]),
    "tem_conv_packed_size": (c_i64, [c_int] * 5),
    "tem_conv_pack_weights": (c_int, [c_vp, c_vp] + [c_int] * 7 + [c_vp]),
    "tem_conv_pack_weights_batch": (c_int, [c_vp, c_int, c_i64, c_vp]),
    "tem_conv_pack_weights_tiles": (c_int, [c_vp, c_int, c_i64, c_vp]),
    "tem_conv_unpack_wgrad": (c_int, [c_vp, c_vp] + [c_int] * 5 + [c_vp]),
    "tem_conv3d_fwd_ws": (c_i64, [c_int] * 10),
    "tem_conv3d_fwd": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64]
                       + [c_int] * 11 + [c_vp]),
    "tem_conv3d_fwd_stat_blocks": (c_i64, [c_int] * 10),
    "tem_conv3d_fwd_kernel": (c_int, [c_int] * 10),
    "tem_conv3d_fwd_stat_blocks_ld": (c_i64, [c_int] * 10 + [c_i64] * 3 + [c_int]),
    "tem_conv3d_fwd_kernel_ld": (c_int, [c_int] * 10 + [c_i64] * 3 + [c_int]),
    "tem_conv3d_fwd_stats": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64]
                             + [c_int] * 11 + [c_vp, c_i64, c_vp]),
    # dispatch queries of the VALU family for the arguments of an actual launch (launch nothing); inst: host int[4] or None
    "tem_conv3d_fwd_valu_path": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64] + [c_int] * 12
                                 + [ctypes.POINTER(c_int)]),
    # ... of the matrix-core family: (x, x_ld, scale, shift, w, bias, y, y_ld, ref, ref_ld, ws_bytes, N .. kw, act, use_mfma, in_amax,
    # ref_coef, has_stat, x_cs, y_cs, TemByproducts* (host, read only), inst: host int[TEM_MFMA_INST_N] or None)
    "tem_conv3d_fwd_mfma_path": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i64] + [c_int] * 11
                                 + [c_vp, c_vp, c_int, c_i64, c_i64, c_vp, ctypes.POINTER(c_int)]),
    "tem_conv3d_wgrad_path": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_int, c_i64] + [c_int] * 11),
    "tem_conv3d_wgrad_ws": (c_i64, [c_int] * 10),
    "tem_conv3d_wgrad": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64] + [c_int] * 11 + [c_vp]),
    "tem_conv1x1_out_bwd_ok": (c_int, [c_int] * 2),
    "tem_conv1x1_out_bwd_ws": (c_i64, [c_int] * 2),
    "tem_conv1x1_out_bwd": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp]),
    "tem_conv3d_wgrad_gmax_ok": (c_int, [c_int] * 10),
    "tem_conv3d_wgrad_gmax": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]
                              + [c_int] * 10 + [c_vp]),
    "tem_conv3d_wgrad_gscaled_ok": (c_int, [c_int] * 9),
    "tem_conv3d_wgrad_cs_ok": (c_int, [c_int] * 10 + [c_i64]),
    "tem_conv3d_wgrad_gscaled": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]
                                 + [c_int] * 9 + [c_vp]),
    "tem_absmax": (c_int, [c_vp, c_i64, c_int, c_i64, c_vp, c_vp]),
    "tem_norm_bwd_from_partials": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_i64,
                                           c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    # (..., in_amax, ref_coef, TemByproducts*, stream) / (..., g_amax_in, g_amax_out, ws, ws_bytes, dims, use_mfma, TemByproducts*, stream)
    "tem_conv3d_fwd_ex": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64] + [c_int] * 11
                          + [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp]),
    "tem_conv3d_wgrad_ex": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]
                            + [c_int] * 10 + [c_i64, c_vp, c_vp]),
    "tem_conv3d_fwd_gscaled": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64] + [c_int] * 9 + [c_vp]),
    "tem_conv3d_fwd_refnorm": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64] + [c_int] * 10 + [c_vp]),
    "tem_norm_ws": (c_i64, [c_int, c_i64, c_int]),
    "tem_conv3d_wgrad_gnorm_ok": (c_int, [c_int] * 6),
    "tem_conv3d_wgrad_gnorm": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64]
                               + [c_int] * 10 + [c_vp]),
    "tem_conv3d_wgrad_sums_ok": (c_int, [c_int] * 10),
    "tem_conv3d_wgrad_sums": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64]
                              + [c_int] * 10 + [c_vp]),
    "tem_norm_bwd_from_sums": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                                       c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_norm_stats": (c_int, [c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_float,
                               c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_norm_finalize_partials": (c_int, [c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_float,
                                           c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tem_norm_bwd": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_int,
                             c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_maxpool3d_fwd": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp]),
    "tem_maxpool3d_fwd_stat_blocks": (c_i64, [c_int] * 5),
    "tem_maxpool3d_fwd_stats": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_i64, c_vp]),
    "tem_maxpool3d_bwd": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_vp, c_i64] + [c_int] * 8 + [c_vp]),
    "tem_maxpool3d_bwd_norm": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_vp, c_i64] + [c_int] * 8
                               + [c_vp, c_i64, c_vp, c_vp]),
    "tem_upsample_bwd_norm": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "tem_norm_bwd_coef": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_upsample_stats": (c_int, [c_vp, c_i64] + [c_int] * 8 + [c_vp, c_vp]),
    "tem_norm_finalize_partials2": (c_int, [c_vp, c_i64, c_int, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_float,
                                            c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tem_upsample_fwd": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp]),
    "tem_upsample_fwd_stats_ok": (c_int, [c_int] * 4),
    "tem_upsample_fwd_stats": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_vp]),
    "tem_upsample_bwd": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp]),
    "tem_dice_ws": (c_i64, [c_int, c_i64, c_int]),
    "tem_dice_sums": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_i64,
                              c_vp, c_vp, c_i64, c_vp]),
    "tem_dice_finalize": (c_int, [c_vp, c_int, c_double, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tem_dice_grad": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_int,
                              c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_i64, c_vp]),
    "tem_dice_sums2": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_i64, c_vp, c_vp, c_i64,
                               c_int, c_vp]),
    "tem_dice_finalize2": (c_int, [c_vp, c_int, c_int, c_double, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tem_dice_grad2": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_int,
                               c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_i64, c_int, c_float, c_float, c_vp]),
    "tem_dice_sums_pair": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_i64,
                                   c_vp, c_vp, c_i64, c_vp]),
    # (x, labels, mask, N, S, act, mask_mode, mask_sample, t_hi, t_lo, st, stream)
    "tem_pseudo_label_st": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_int, c_int, c_float, c_float, c_int, c_vp]),
    "tem_label_count_parts": (c_int, [c_i64, c_int]),
    # (labels, n, threshold, partials, parts, st, stream) / (labels, out, n, threshold, source0, source1, partials, parts, st, stream)
    "tem_label_count_st": (c_int, [c_vp, c_i64, c_float, c_vp, c_int, c_int, c_vp]),
    "tem_distribution_align_st": (c_int, [c_vp, c_vp, c_i64, c_float, c_float, c_float, c_vp, c_int, c_int, c_vp]),
    # (src, dst, codes_dev, N, planes, H, W, elem_bytes, stream) / (src, dst, code, N, planes, H, W, elem_bytes) -> 0 vector
    # stream, 1 scalar stream, 2 tile, 3 packed tile, -1 refused
    "tem_dihedral2d": (c_int, [c_vp, c_vp, c_vp] + [c_int] * 5 + [c_vp]),
    "tem_dihedral2d_path": (c_int, [c_vp, c_vp] + [c_int] * 6),
    "tem_adamw_step": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_float, c_float, c_float, c_float, c_float, c_i64,
                               c_float, c_vp]),
    "tem_adamw_hyper": (c_int, [c_vp, c_float, c_float, c_float, c_float, c_float, c_i64, c_float]),
    "tem_adamw_step_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "tem_adamw_step_tab": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "tem_amp_unscale_dev": (c_int, [c_vp, c_i64, c_vp, c_vp]),
    "tem_amp_update_dev": (c_int, [c_vp, c_float, c_float, c_int, c_vp]),
    "tem_ema_update": (c_int, [c_vp, c_vp, c_i64, c_float, c_vp]),
    "tem_amp_unscale": (c_int, [c_vp, c_i64, c_float, c_vp, c_vp]),
    "tem_boundary_target": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "tem_boundary_target_mode": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tem_affinity_target": (c_int, [c_vp, c_vp, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, c_int, c_i64,
                                    c_int, c_int, c_int, c_vp]),
    "tem_pod_cc_roots": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "tem_pod_cc_assign": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_i64, c_vp]),
    "tem_pod_seq_flag": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp]),
    "tem_pod_seq_assign": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_i64, c_vp]),
    "tem_pod_size_keep": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_vp]),
    "tem_pod_size_apply": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_vp]),
    "tem_pod_ws": (c_i64, [c_int, c_i64, c_int, c_int]),
    "tem_pod_targets": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_float), c_int, c_float,
                                c_vp, c_i64, c_vp]),
    "tem_vector_edt": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    "tem_distance_targets_ws": (c_i64, [c_int, c_int]),
    "tem_distance_targets": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_vp, c_i64,
                                     c_vp]),
    "tem_boundary_target_masked": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_i64, c_int, c_vp]),
    "tem_onehot_target": (c_int, [c_vp, ctypes.POINTER(c_i64), c_int, c_vp, c_int, c_i64, c_vp]),
    "tem_dist_loss_ws": (c_i64, []),
    "tem_dist_loss_fwd": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_int, c_i64, c_int, c_int,
                                  c_double, c_double, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_dist_loss_grad": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_int, c_i64,
                                   c_int, c_vp]),
    "tem_cldice_ws": (c_i64, [c_int, c_int, c_i64, c_int, c_int]),
    "tem_cldice_step": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp] + [c_int] * 7 + [c_vp]),
    "tem_cldice_dilate_bwd": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp] + [c_int] * 6 + [c_vp]),
    "tem_cldice_erode_bwd": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64]
                             + [c_int] * 6 + [c_vp]),
    "tem_cldice_sums": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_i64,
                                c_vp, c_i64, c_vp]),
    "tem_cldice_finalize": (c_int, [c_vp, c_double, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tem_cldice_grad": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_int, c_int, c_i64, c_vp]),
    "tem_nchw_to_nhwc": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_i64, c_vp]),
    "tem_nhwc_to_nchw": (c_int, [c_vp, c_i64, c_vp, c_int, c_int, c_i64, c_vp]),
    "tem_standardize": (c_int, [c_vp, c_vp, c_int, c_i64, c_float, c_vp, c_i64, c_vp]),
    "tem_spoco_ws": (c_i64, [c_int, c_int, c_i64, c_int, c_int, c_int]),
    "tem_label_range": (c_int, [c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "tem_spoco_cluster_means": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_spoco_pull": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_float, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_spoco_means_terms": (c_int, [c_vp, c_int, c_int, c_float, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_spoco_instance_dice": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_int, c_vp, c_float, c_float, c_vp,
                                        c_vp, c_i64, c_vp]),
    "tem_spoco_push": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_float, c_vp, c_float, c_vp, c_i64,
                               c_vp, c_vp, c_i64, c_vp]),
    "tem_spoco_embed_grad": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
                             + [c_float] * 6 + [c_vp, c_i64, c_int, c_vp, c_i64, c_vp]),
    "tem_zero_count": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "tem_zero_select": (c_int, [c_vp, c_i64, c_vp, c_vp, c_int, c_vp, c_vp]),
    "tem_spoco_consistency": (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_int, c_float, c_float, c_vp,
                                      c_float, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "tem_affinity_side": (c_int, [c_vp, c_i64, c_vp, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int, c_float,
                                  c_float, c_vp, c_float, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "tem_flip3d": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tem_affine_warp3d": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tem_elastic_field": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_float, c_float, c_vp, c_vp]),
    "tem_elastic_warp2d": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_vp]),
    "tem_block_load_reflect": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int] + [ctypes.POINTER(c_int)] * 4 + [c_vp]),
    "tem_block_store_inner": (c_int, [c_vp, ctypes.POINTER(c_int), c_vp, c_int, c_int, c_int, c_int, c_vp]
                              + [ctypes.POINTER(c_int)] * 3 + [c_vp]),
    "tem_accumulate_channels": (c_int, [c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_i64] + [c_int] * 5 + [c_vp]),
    "tem_act_bwd": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp]),
    # round 5: activation storage types (TEM_ST_*) as explicit arguments
    "tem_maxpool3d_fwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_i64, c_int, c_vp]),
    "tem_maxpool3d_bwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_vp, c_i64] + [c_int] * 8
                             + [c_vp, c_i64, c_vp, c_vp, c_int, c_vp]),
    "tem_upsample_fwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_int, c_vp]),
    "tem_upsample_bwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_i64, c_vp, c_i64, c_int, c_vp]),
    "tem_upsample_stats_st": (c_int, [c_vp, c_i64] + [c_int] * 8 + [c_vp, c_int, c_vp]),
    # dispatch queries: 0 gather<1>, 1 gather<4>, 2 factor-2 <.., 4>, 3 factor-2 <.., 8>, -1 refused
    "tem_upsample_fwd_path": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_int, c_int]),
    "tem_upsample_bwd_path": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_vp, c_i64, c_int]),
    # 0 <1>, 1 <4>, 2 <8>, 3 packed 16-bit fz = 1, 4 packed 16-bit fz = 2, -1 refused
    "tem_maxpool3d_fwd_path": (c_int, [c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_int, c_int]),
    "tem_maxpool3d_bwd_path": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64] + [c_int] * 8 + [c_int, c_int, c_int]),
    "tem_norm_stats_st": (c_int, [c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_float,
                                  c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_vp]),
    "tem_norm_bwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_i64,
                                c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_int, c_vp]),
    # dispatch queries (launch nothing): out int64[5] = vec, rows, threads, nblk, vper / int64[4] = vec, threads, grid_x, fast; -1 refused
    "tem_norm_reduce_geom": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_int, c_int, ctypes.POINTER(c_i64)]),
    "tem_norm_apply_geom": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int, c_i64, c_int, c_int, c_int, ctypes.POINTER(c_i64)]),
    "tem_conv3d_wgrad_gnorm_st": (c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64]
                                  + [c_int] * 12 + [c_vp]),
    "tem_conv1x1_out_bwd_st": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int,
                                       c_vp, c_int, c_int, c_vp]),
    # raw normalisation and contrast (csrc/rawnorm.hip); `ranks`, `values`, `t` are HOST arrays
    "tem_rawnorm_ws": (c_i64, [c_int, c_i64, c_int]),
    "tem_row_minmax": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tem_row_select": (c_int, [c_vp, c_int, c_i64, ctypes.POINTER(c_i64), c_int, c_vp, c_vp, c_i64, c_vp]),
    "tem_rawnorm_fill": (c_int, [c_vp, ctypes.POINTER(c_float), c_i64, c_vp]),
    "tem_rawnorm_minmax_coef": (c_int, [c_vp, c_vp, c_int, c_float, c_vp, c_vp, c_vp]),
    "tem_rawnorm_percentile_coef": (c_int, [c_vp, ctypes.POINTER(c_float), c_int, c_float, c_vp, c_vp, c_vp, c_vp]),
    "tem_rawnorm_apply": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_float, c_float, c_vp]),
    "tem_rawnorm_contrast": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_float, c_int, c_float, c_float, c_vp]),
    # noise and blur raw augmentations (csrc/rawaug.hip): (..., seed, stream row of the first data row, clip, lo, hi, stream)
    "tem_rawaug_philox_words": (c_int, [c_vp, c_u64, c_u32, c_u64, c_u32, c_i64, c_vp]),
    "tem_rawaug_gauss_noise": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_u64, c_u32, c_int, c_float, c_float, c_vp]),
    "tem_rawaug_poisson_add": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_u64, c_u32, c_int, c_float, c_float, c_vp]),
    "tem_rawaug_poisson_scaled": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_vp, c_u64, c_u32, c_int, c_float, c_float, c_vp]),
    "tem_rawaug_blur2d": (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp]),
    "tem_rawaug_blur_z": (c_int, [c_vp, c_vp, c_i64, c_int, c_i64, c_vp, c_int, c_vp]),
    # seeded watershed (csrc/watershed.hip): (rank, order, markers, marker_bytes, mask, out, rounds_out, N, D, H, W, ws, ws_bytes, stream)
    "tem_watershed_rounds": (c_int, [c_i64]),
    "tem_watershed_ws": (c_i64, [c_int, c_i64]),
    "tem_watershed": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_i64, c_vp]),
    # mutex watershed (csrc/mws.hip): (mask, edge_valid, offsets, n_attractive, N, C, D, H, W, ws, ws_bytes, stream) /
    # (aff, offsets, n_attractive, N, C, D, H, W, ws, ws_bytes, table, slots, first, rounds, stream) /
    # (out, N, C, D, H, W, ws, ws_bytes, stream)
    "tem_mws_ws": (c_i64, [c_int] * 5),
    "tem_mws_table_slots": (c_i64, [c_i64]),
    "tem_mws_init": (c_int, [c_vp, c_vp, c_vp, c_int] + [c_int] * 5 + [c_vp, c_i64, c_vp]),
    "tem_mws_run": (c_int, [c_vp, c_vp, c_int] + [c_int] * 5 + [c_vp, c_i64, c_vp, c_i64, c_int, c_int, c_vp]),
    "tem_mws_labels": (c_int, [c_vp] + [c_int] * 5 + [c_vp, c_i64, c_vp]),
    # label overlaps and instance-segmentation scores (csrc/overlap.hip): (sorted, flag, N, V, stream) /
    # (sorted, rank, pa, pb, n_ab, npairs, n_a, n_b, N, V, ws, ws_bytes, stream) /
    # (pa, pb, n_ab, npairs, n_a, n_b, threshold, rec, best_a, best_b, N, V, ws, ws_bytes, stream)
    "tem_overlap_ws": (c_i64, [c_int, c_i64]),
    "tem_overlap_flag": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp]),
    "tem_overlap_table": (c_int, [c_vp] * 8 + [c_int, c_i64, c_vp, c_i64, c_vp]),
    "tem_overlap_scores": (c_int, [c_vp] * 6 + [c_double, c_vp, c_vp, c_vp, c_int, c_i64, c_vp, c_i64, c_vp]),
    # EM defect augmentation (csrc/defect.hip): plan int32 [S][4], rec int32 [D][8], tables int32 (include/tem_hip.h)
    "tem_defect_mean": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_vp]),
    "tem_defect_apply": (c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tem_defect_flow": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_u64, c_float, c_vp, c_int, c_vp]),
    "tem_defect_prefilter": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tem_defect_warp": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_u64, c_double, c_vp]),
    # patch supply from device-resident volumes (csrc/patch.hip): vols int64 [V][6], boxes int32 [M][8] (include/tem_hip.h)
    "tem_patch_count": (c_int, [c_vp, c_vp, c_int, c_int, c_i64, c_i64, c_vp, c_vp]),
    "tem_patch_hist": (c_int, [c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_vp]),
    "tem_patch_hist_path": (c_int, [c_int]),
    "tem_patch_hist_reduce": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "tem_patch_gather": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
}

_lib = None


BP_OUT_AMAX, BP_NORM_COEF, BP_NORM_SUMS = 1, 2, 4


class Byproducts(ctypes.Structure):
    """include/tem_hip.h: TemByproducts -- the optional by-products of ONE call, passed to a *_ex entry point"""
    _fields_ = [("out_amax", c_vp), ("coef_G", c_int), ("coef_mean", c_vp), ("coef_rstd", c_vp), ("coef", c_vp),
                ("sums_x", c_vp), ("sums_x_ld", c_i64), ("sums_mean", c_vp), ("sums_rstd", c_vp), ("sums_G", c_int),
                ("sums_part", c_vp), ("sums_nblk", c_i64), ("delivered", ctypes.c_uint)]


class TemError(RuntimeError):
    """HIP launch / runtime failure inside libtem_hip.so."""


def build(verbose=False):
    """Compile libtem_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    # MAX_JOBS (the convention of torch extension builds) sets the job count; otherwise at most 16: os.cpu_count() is the
    # whole host's, not this process's share of it
    jobs = int(os.environ.get("MAX_JOBS") or min(os.cpu_count() or 4, 16))
    cmd = ["make", "-C", CSRC, "-j", str(jobs)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise RuntimeError("building libtem_hip.so failed (see output above)")
    return LIB_PATH


def load():
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libtem_hip.so not found at {LIB_PATH}: the MI355X kernels are not built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or make -C torch_em_amd/csrc). "
            "There is no CPU fallback for this path."
        )
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so both share one HIP runtime)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("TEM_LIB"):   # an older A/B build of the C-ABI (developer override): the symbol stays unavailable
                continue
            raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it (make -C torch_em_amd/csrc)")
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    # dispatch options of the library (tem_set_option) can be preset from the HOST environment as TEM_OPT_<NAME>=<int>;
    # the library itself never reads the environment
    for key, val in os.environ.items():
        if key.startswith("TEM_OPT_"):
            check(lib.tem_set_option(key[8:].lower().encode(), int(val)), key)
    return lib


def set_option(name, value):
    """Select a kernel variant (names: include/tem_hip.h, tem_set_option)."""
    check(load().tem_set_option(name.encode(), int(value)), "tem_set_option")


def get_option(name):
    out = c_i64(0)
    check(load().tem_get_option(name.encode(), ctypes.byref(out)), "tem_get_option")
    return int(out.value)


_tls = threading.local()


def launch_on(idx):
    """Make device `idx` current for the launch being assembled; `check()` -- which wraps every launch -- puts the
    caller's device back, so an op on a `cuda:1` tensor does not move the process's current device for good."""
    import torch
    cur = torch.cuda.current_device()
    if idx is not None and idx != cur:
        if getattr(_tls, "restore", None) is None:
            _tls.restore = cur
        torch.cuda.set_device(idx)


def check(rc, what=""):
    """Map a C-ABI return code to the exception the reference raises for the same mistake."""
    prev = getattr(_tls, "restore", None)
    if prev is not None:
        import torch
        _tls.restore = None
        torch.cuda.set_device(prev)
    if rc == 0:
        return
    msg = load().tem_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(msg or f"{what}: invalid argument")
    raise TemError(f"{what}: {msg} (rc={rc})")
