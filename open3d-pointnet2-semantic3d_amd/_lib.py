"""ctypes binding of libpn2_hip.so (the C ABI declared in include/pn2_abi.h).

There is deliberately NO fallback: if the HIP library cannot be loaded the
import fails loudly.  The library must be loaded after `import torch` so that it
binds to the HIP runtime torch already mapped (same soname libamdhip64.so.7);
tensors and streams are then shared with torch without copies.
"""
import ctypes
import os
import sys

import torch  # noqa: F401  (must precede CDLL: maps torch's libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PN2_HIP_LIBRARY: load another build of the same ABI instead (the tuning build of the A/B scripts under tools/)
LIB_PATH = os.environ.get("PN2_HIP_LIBRARY") or os.path.join(_HERE, "libpn2_hip.so")

c_int, c_float, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

# name -> argtypes, in the order of include/pn2_abi.h
SIGNATURES = {
    "pn2_farthest_point_sample": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_fps_gather": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_fps_nested": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_fps_nested_ld": [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_coarse_geometry": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "pn2_prob_sample": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_fps_large": [c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_gather_point": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_gather_point_grad": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_query_ball_point": [c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_query_ball_point_ld": [c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_query_ball_point_kernel": [c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_void_p],
    "pn2_query_ball_point_multi": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int, c_void_p],
    "pn2_selection_sort": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_group_point": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_group_point_grad": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_three_nn": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_three_nn_ld": [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_three_interpolate": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_three_interpolate_grad": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_group_point_grad_ws": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t,
                                c_void_p],
    "pn2_three_interpolate_grad_ws": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      ctypes.c_size_t, c_void_p],
    "pn2_linear": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "pn2_linear_wgrad": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_forward": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_backward": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                             c_int, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_set_sa_row_packing": [c_int],
    "pn2_sa_mlp_max_fused": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_sa_mlp_max_fused_ld": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_sa_mlp_max_fused_bf16": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_sa_mlp_rows_fused": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_fp_interp_concat": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_int, c_void_p],
    "pn2_mlp_chain": [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    "pn2_fp_mlp_fused": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_interpolate_label_with_color": [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         ctypes.c_size_t, c_void_p],
    "pn2_sa_group_concat": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p],
    "pn2_mlp_wide": [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "pn2_sa_mlp_wide": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                        c_void_p, c_int, c_void_p, c_void_p],
    "pn2_fp_mlp_wide": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                        c_void_p, c_void_p, c_void_p],
    "pn2_multi_copy": [c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_multi_copy_fill": [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_scatter_plan_build": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_scatter_plan_build_multi": [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     ctypes.c_size_t, c_void_p],
    "pn2_scatter_plan_apply": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p],
    "pn2_scatter_plan_apply_multi": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p],
    "pn2_linear_bn_stats": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_linear_wgrad_accumulate": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_dgrad": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_forward_deferred": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                     c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_bn_stats_xf": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p,
                               c_int, c_void_p],
    "pn2_linear_wgrad_accumulate_xf": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_sa_hoist_rows": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p],
    "pn2_fp_hoist_rows": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_sa_hoist_rows_bn": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_fp_hoist_rows_bn": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_sa_hoist_rows_multi_bn": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_dgrad_bn_grad_stats": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_linear_bn_stats_fin": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p,
                                c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_dgrad_fin": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                             ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_forward_mode": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                 c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_backward_mode": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_int, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p],
    "pn2_sa_first_layer_bn": [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_bwd_fused": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_linear_narrow": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_grad_constants": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_bn_relu_forward_pool": [ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_int,
                                 c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p],
    "pn2_linear_dgrad_gx": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_linear_wgrad_gx": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_weighted_ce_forward": [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_weighted_ce_backward": [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p],
    "pn2_confusion_update": [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p],
    "pn2_dropout": [ctypes.c_longlong, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_dropout_grad": [ctypes.c_longlong, c_void_p, c_void_p, c_float, c_void_p, c_void_p],
    "pn2_relu_grad": [ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_adam_step": [ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_momentum_step": [ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_scene_extract_z_box": [c_int, c_void_p, c_int, c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int,
                                c_void_p, c_void_p, c_void_p],
    "pn2_scene_sample": [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_double,
                         ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_fp_mlp_fused_pre": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p],
    "pn2_fp_mlp_fused_pre_ld": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p],
    "pn2_fp_mlp_fused_pre_schedule": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "pn2_sa_mlp_fused_pre": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                             c_void_p, c_int, c_void_p, c_void_p],
    "pn2_fp_mlp_wide_pre": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p],
    "pn2_sa_mlp_wide_pre": [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                            c_void_p, c_int, c_void_p, c_void_p],
    "pn2_ball_query_bin": [c_int, c_int, c_float, c_void_p, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_ball_query_bin_ld": [c_int, c_int, c_float, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_query_ball_point_binned": [c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p],
    "pn2_group_pool": [ctypes.c_longlong, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_group_pool_grad": [ctypes.c_longlong, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "pn2_voxel_downsample": [c_int, c_void_p, c_void_p, c_void_p, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, ctypes.c_size_t, c_void_p],
    "pn2_dataset_workspace_size": [c_int, c_int, c_void_p],
    "pn2_dataset_sample": [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int, c_void_p, c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p],
}
PN2_EUNSUP = -4
# state of a batch-norm workspace when a call arrives: PN2_BN_WS_* of include/pn2_abi.h (the stats_mode argument)
BN_WS_UNCLEARED, BN_WS_ZEROED, BN_WS_SUMMED, BN_WS_FOLDED = range(4)
# workspace-size queries (-> size_t): name -> number of int arguments
_SIZE_QUERIES = {"pn2_fps_large_workspace_bytes": 2, "pn2_ball_query_bin_bytes": 1, "pn2_interpolate_label_workspace_bytes": 1,
                 "pn2_three_interpolate_grad_workspace_bytes": 3, "pn2_scatter_plan_bytes": 3,
                 "pn2_group_point_grad_workspace_bytes": 4, "pn2_voxel_downsample_workspace_bytes": 1, "pn2_bn_workspace_bytes": 1}
# What the benchmark trace decodes besides the numeric arguments: entry point -> (index of nlayers, index of the host widths[]
# array in the argument list -- both None when there is none --, trace key, positions AMONG THE NUMERIC ARGUMENTS to drop).  An
# in-place (row-strided) *_ld call is the dense entry point's kernel: recorded under the dense name with its strides dropped.
_TRACE_ARGS = {"pn2_sa_mlp_max_fused": (9, 10, None, ()), "pn2_sa_mlp_rows_fused": (9, 10, None, ()),
               "pn2_sa_mlp_max_fused_bf16": (9, 10, None, ()), "pn2_fp_mlp_fused": (9, 10, None, ()),
               "pn2_fp_mlp_wide_pre": (8, 9, None, ()), "pn2_sa_mlp_wide_pre": (8, 9, None, ()),
               "pn2_sa_mlp_fused_pre": (8, 9, None, ()), "pn2_fp_mlp_fused_pre": (8, 9, None, ()),
               "pn2_fp_mlp_fused_pre_schedule": (8, 9, None, ()), "pn2_mlp_chain": (3, 4, None, ()),
               "pn2_mlp_wide": (4, 5, None, ()), "pn2_fp_mlp_wide": (9, 10, None, ()), "pn2_sa_mlp_wide": (9, 10, None, ()),
               "pn2_fps_nested_ld": (None, None, "pn2_fps_nested", (3,)),
               "pn2_query_ball_point_ld": (None, None, "pn2_query_ball_point", (5,)),
               "pn2_three_nn_ld": (None, None, "pn2_three_nn", (3,)),
               "pn2_ball_query_bin_ld": (None, None, "pn2_ball_query_bin", (3,)),
               "pn2_sa_mlp_max_fused_ld": (11, 12, "pn2_sa_mlp_max_fused", (5, 6)),
               "pn2_fp_mlp_fused_pre_ld": (9, 10, "pn2_fp_mlp_fused_pre", (4,))}


class Pn2Error(RuntimeError):
    pass


def _load():
    # Build in-tree with hipcc when the library is missing OR older than its sources (cross-compiles without a GPU);
    # never fall back to CPU code.  One process per GPU may import concurrently (torch.distributed.run): the check
    # and the build run under a file lock, and build.py links to a temporary file that is renamed into place, so no
    # rank can dlopen a half-written library.  An up-to-date library is loaded without touching the tree (it may be
    # read-only to the user who runs it); the lock is taken only when a build may be needed.
    import fcntl
    from . import build as _build
    if not os.environ.get("PN2_HIP_LIBRARY") and _build._stale():
        if not os.access(_HERE, os.W_OK) and os.path.exists(_build.LIB):
            sys.stderr.write("pn2: %s is older than its sources but %s is not writable: loading the library as built\n"
                             % (_build.LIB, _HERE))
        else:
            with open(os.path.join(_HERE, ".build.lock"), "a") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    if _build._stale():  # another process may have built it while this one waited
                        _build.build()
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise ImportError("cannot load the HIP extension %s: %s -- there is no CPU fallback; "
                          "build it with `python open3d-pointnet2-semantic3d_amd/build.py`" % (LIB_PATH, e))
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and the library disagree
        fn.argtypes = argtypes
        fn.restype = c_int
    for name, nargs in _SIZE_QUERIES.items():
        fn = getattr(lib, name)
        fn.argtypes = [c_int] * nargs
        fn.restype = ctypes.c_size_t
    lib.pn2_abi_version.restype = c_int
    lib.pn2_build_info.restype = ctypes.c_char_p
    lib.pn2_strerror.restype = ctypes.c_char_p
    lib.pn2_strerror.argtypes = [c_int]
    if lib.pn2_abi_version() != 2:
        raise ImportError("libpn2_hip.so ABI version mismatch")
    return lib


_raw = _load()


# entry points that mutate caller state beyond their outputs (moving averages, optimizer slots): never launched twice by the dup hook
_STATEFUL = frozenset({"pn2_bn_relu_forward", "pn2_linear_bn_stats",
                       "pn2_bn_relu_forward_pool", "pn2_bn_relu_forward_deferred", "pn2_linear_bn_stats_xf", "pn2_linear_wgrad_gx",
                       "pn2_linear_wgrad_accumulate_xf", "pn2_bn_grad_constants", "pn2_linear_dgrad_gx", "pn2_linear_dgrad_fin",
                       "pn2_linear_bn_stats_fin", "pn2_bn_relu_forward_mode", "pn2_sa_first_layer_bn", "pn2_sa_hoist_rows_bn", "pn2_fp_hoist_rows_bn", "pn2_sa_hoist_rows_multi_bn", "pn2_linear_bwd_fused", "pn2_linear_dgrad_bn_grad_stats",
                       "pn2_adam_step", "pn2_momentum_step", "pn2_linear_wgrad_accumulate"})


class _LibProxy:
    """Attribute proxy over the ctypes library.  When `trace` is a list, every pn2_* launch is
    bracketed by two events on torch's current stream (the stream the kernel is launched on) and
    (name, numeric_args, start_event, end_event) is appended -- bench.py derives per-kernel durations
    and roofline numbers from it.  With trace=None (default) calls go straight through."""

    def __init__(self, raw):
        self._raw = raw
        self.trace = None
        self.dup = ()  # experiment hook: entry points launched twice (marginal-cost ablation, bench.py --dup)

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if name not in SIGNATURES:
            return fn

        def call(*args):
            if name in self.dup and name not in _STATEFUL:
                fn(*args)  # a pure function of its inputs: the second launch rewrites the same values
            if self.trace is None:
                return fn(*args)
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn(*args)
            e.record()
            ints = [a for a in args if isinstance(a, (int, float))]
            key = name
            if name in _TRACE_ARGS:
                nl_at, w_at, dense, drop = _TRACE_ARGS[name]
                key = dense or name
                ints = [v for i, v in enumerate(ints) if i not in drop]
                if w_at is not None:  # decode the host-side widths[] array for flop accounting
                    wp = ctypes.cast(args[w_at], ctypes.POINTER(c_int))
                    ints += [wp[i] for i in range(args[nl_at])]
            elif name == "pn2_coarse_geometry":  # (b, n0, nlev, npoint[], radius[], nsample[], ...): decode the host arrays
                ints += list(args[3]) + list(args[5])
            self.trace.append((key, tuple(ints), s, e))
            return rc

        call.__name__ = name
        setattr(self, name, call)  # cache
        return call


lib = _LibProxy(_raw)


def strerror(code):
    return lib.pn2_strerror(int(code)).decode()


def check(code, what):
    if code != 0:
        raise Pn2Error("%s failed: %s (code %d)" % (what, strerror(code), code))


def ptr(t, byte_offset=0):
    """device pointer of a tensor (None -> NULL), optionally `byte_offset` bytes into it."""
    return None if t is None else c_void_p(t.data_ptr() + byte_offset)


def rows_in_place(t):
    """(tensor, ld) for a (b, n, c) float32 tensor the *_ld entry points can read where it lies: rows `ld` floats apart, clouds
    n * ld floats apart -- a dense tensor (ld = c) or a column block of a wider dense one (point_cloud[:, :, 0:3] of a (b,n,6)
    batch: ld = 6).  Anything else -- other layouts, other dtypes (ld counts FLOATS) -- is copied dense: ld = c elements."""
    t = t.detach()
    if t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(0) == t.shape[1] * t.stride(1) \
            and t.data_ptr() % 4 == 0:
        return t, int(t.stride(1))
    t = t.contiguous()
    return t, int(t.shape[2])


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(name, where, *args, may_refuse=False, stream=True):
    """Call entry point `name` with `args` + torch's current stream (stream=False: a host-side query that takes none), on the
    device of `where` (a tensor or a device).  The entry point is looked up on `lib` at call time (the trace / dup hooks see it).
    -> True; with may_refuse, False when the library reports the configuration as unsupported (PN2_EUNSUP).  Every other failure
    raises Pn2Error naming the entry point."""
    with torch.cuda.device(getattr(where, "device", where)):
        rc = getattr(lib, name)(*args, stream_ptr()) if stream else getattr(lib, name)(*args)
    if may_refuse and rc == PN2_EUNSUP:
        return False
    check(rc, name)
    return True


def nbytes(t):
    return t.numel() * t.element_size()


# Host arrays for the entry points that read widths[] / pointer tables: ctypes arrays, accepted as they are where the argtype is
# c_void_p.  The caller holds them until the call has returned (the library reads them before it returns).
def int_array(values):
    return (c_int * len(values))(*[int(v) for v in values])


def float_array(values):
    return (c_float * len(values))(*[float(v) for v in values])


def u64_array(values):
    """64-bit unsigned: byte counts and offsets (size_t), raw 64-bit payloads"""
    return (ctypes.c_uint64 * len(values))(*[int(v) for v in values])


def ptr_table(tensors):
    """host table of device pointers (None -> NULL)"""
    return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def layer_arrays(ws, bs):
    """-> nlayers, widths[], weight pointers, bias pointers of a stack of dense layers (ws[i]: (cin_i, cout_i))"""
    return len(ws), int_array([w.shape[1] for w in ws]), ptr_table(ws), ptr_table(bs)


def require_cuda(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("pn2 ops run on the MI355X only: got a %s tensor (there is no CPU path in the "
                             "product; the CPU oracle lives under oracle/ for tests)" % t.device)
