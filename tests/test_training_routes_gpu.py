"""Which entry points one training forward + backward of the SA / MSG / FP modules and the dense layers launches, at the smallest
shapes on both sides of every host-side threshold of the training layer path and with every training switch off (util/tf_util.py:
the switch block, _dense_bn_gemm, _bn_tail, _BnLink; util/pointnet_util.py: the first-layer forms, _defer_after).  The cases and
the traced call are those of tools/training_routes.py; the sequences below are the ones the commit before the shared batch-norm
tail launched (its output is profiles/r10_training_routes_parent.txt), forward then backward in the autograd engine's order.  Only
the entry points are pinned, not the arguments or the hashes: later tuning stays possible, a change of route has to be made here
too."""
import pytest

from tools import training_routes

pytestmark = pytest.mark.gpu

# case -> the pn2_* entry points of one forward + backward, in launch order (a refused call is traced too)
EXPECTED = {
    "sa_c3_32_32_64_rows4096":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "sa_c3_32_32_64_rows2048":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused "
        "pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "sa_c3_64_pooled_first":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_pool pn2_bn_grad_constants "
        "pn2_linear_wgrad_gx",
    "sa_c64_64_64_128_plan_rows4096":
        "pn2_linear pn2_sa_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused "
        "pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate "
        "pn2_linear_wgrad_accumulate",
    "sa_c64_64_64_128_plan_rows32768":
        "pn2_linear pn2_sa_hoist_rows_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused pn2_bn_relu_backward_mode "
        "pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "sa_c64_64_64_128_plan_rows32704":
        "pn2_linear pn2_sa_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused "
        "pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate "
        "pn2_linear_wgrad_accumulate",
    "sa_c64_64_64_128_idx_only":
        "pn2_sa_group_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_group_point_grad_ws",
    "sa_c8_32_32_64_grouped":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats_fin "
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused "
        "pn2_linear_bwd_fused pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_group_point_grad_ws",
    "sa_c8_32_32_64_avg":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats_fin "
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_group_pool pn2_group_pool_grad "
        "pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_group_point_grad_ws",
    "msg_two_scales_hoisted":
        "pn2_linear pn2_sa_hoist_rows_multi_bn pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused "
        "pn2_bn_relu_backward_mode pn2_linear_dgrad_fin pn2_linear_wgrad pn2_linear_bwd_fused pn2_bn_relu_backward_mode "
        "pn2_bn_relu_backward_mode pn2_scatter_plan_apply_multi pn2_linear_dgrad pn2_linear_wgrad pn2_linear_wgrad_accumulate "
        "pn2_linear_wgrad_accumulate",
    "msg_one_layer_scale_hoisted":
        "pn2_linear pn2_sa_hoist_rows_multi_bn pn2_bn_relu_forward_pool pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_bn_relu_backward_mode pn2_bn_relu_backward_mode "
        "pn2_scatter_plan_apply_multi pn2_linear_dgrad pn2_linear_wgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "msg_two_scales_no_geometry":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point_multi pn2_group_point pn2_group_point pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_group_point pn2_group_point pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_group_point_grad_ws pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_group_point_grad_ws",
    "fp_c1_3_plan_defer_last_128":
        "pn2_linear pn2_fp_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_bn_relu_backward_mode "
        "pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "fp_c1_3_plan":
        "pn2_linear pn2_fp_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate "
        "pn2_linear_wgrad_accumulate",
    "fp_c1_3_no_plan":
        "pn2_fp_interp_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_three_interpolate_grad_ws",
    "fp_c1_128":
        "pn2_fp_interp_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_scatter_plan_apply",
    "fp_no_points1":
        "pn2_fp_interp_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_scatter_plan_apply",
    "stack_64_64_rows4096":
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_bwd_fused "
        "pn2_linear_bwd_fused",
    "stack_20_32_rows4096":
        "pn2_linear pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx",
    "stack_16_32_rows4096":
        "pn2_linear_narrow pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_bn_relu_backward_mode pn2_linear_dgrad pn2_linear_wgrad",
    "stack_1028_rows64":
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_narrow pn2_bn_relu_forward_mode pn2_bn_relu_backward_mode "
        "pn2_linear_dgrad pn2_linear_wgrad pn2_bn_relu_backward_mode pn2_linear_dgrad pn2_linear_wgrad",
    "dense_relu_no_bn":
        "pn2_linear pn2_relu_grad pn2_linear_dgrad pn2_linear_wgrad pn2_linear_wgrad",
    "conv1d_head_9":
        "pn2_linear_narrow pn2_linear_dgrad pn2_linear_wgrad pn2_linear_wgrad",
    "fanout_two_consumers":
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_bwd_fused pn2_bn_grad_constants "
        "pn2_linear_bwd_fused pn2_bn_grad_constants pn2_linear_bwd_fused",
    "sa_c3_32_32_64_rows4096_no_grad":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool",
    "stack_64_64_rows4096__USE_GEMM_BN_STATS_off":
        "pn2_linear pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants "
        "pn2_linear_bwd_fused pn2_linear_bwd_fused",
    "sa_c3_32_32_64_rows4096__USE_GEMM_BN_STATS_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "stack_64_64_rows4096__USE_BN_FINISH_IN_PRODUCER_off":
        "pn2_linear_bn_stats pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_mode pn2_bn_grad_constants "
        "pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx",
    "sa_c3_32_32_64_rows4096__USE_BN_FINISH_IN_PRODUCER_off":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats "
        "pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_grad_constants "
        "pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_wgrad_gx",
    "sa_c64_64_64_128_plan_rows32768__USE_BN_FINISH_IN_PRODUCER_off":
        "pn2_linear pn2_sa_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_deferred "
        "pn2_linear_bn_stats_xf pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx "
        "pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_relu_backward_mode pn2_scatter_plan_apply "
        "pn2_linear_dgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "msg_two_scales_hoisted__USE_BN_FINISH_IN_PRODUCER_off":
        "pn2_linear pn2_sa_hoist_rows_multi_bn pn2_bn_relu_forward_mode pn2_bn_relu_forward_deferred pn2_linear_bn_stats "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats pn2_bn_relu_forward_pool pn2_linear_bn_stats_xf "
        "pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_gx "
        "pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_relu_backward_mode "
        "pn2_linear_dgrad_bn_grad_stats pn2_linear_wgrad pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx "
        "pn2_bn_relu_backward_mode pn2_bn_relu_backward_mode pn2_scatter_plan_apply_multi pn2_linear_dgrad pn2_linear_wgrad "
        "pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "fp_c1_3_plan_defer_last_128__USE_BN_FINISH_IN_PRODUCER_off":
        "pn2_linear pn2_fp_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_deferred "
        "pn2_linear_bn_stats_xf pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_dgrad_gx "
        "pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_dgrad_gx pn2_linear_wgrad_gx pn2_bn_relu_backward_mode "
        "pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "stack_64_64_rows4096__USE_DGRAD_BN_STATS_off":
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_bwd_fused pn2_bn_grad_constants pn2_linear_bwd_fused",
    "sa_c64_64_64_128_plan_rows4096__USE_DGRAD_BN_STATS_off":
        "pn2_linear pn2_sa_hoist_rows pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_bn_grad_constants pn2_linear_bwd_fused pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad "
        "pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "msg_two_scales_hoisted__USE_DGRAD_BN_STATS_off":
        "pn2_linear pn2_sa_hoist_rows_multi_bn pn2_bn_relu_forward_mode pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_bn_grad_constants pn2_linear_bwd_fused pn2_bn_relu_backward_mode pn2_linear_dgrad "
        "pn2_linear_wgrad pn2_bn_grad_constants pn2_linear_bwd_fused pn2_bn_relu_backward_mode pn2_bn_relu_backward_mode "
        "pn2_scatter_plan_apply_multi pn2_linear_dgrad pn2_linear_wgrad pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "stack_64_64_rows4096__USE_BN_ON_LOAD_off":
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused",
    "sa_c3_32_32_64_rows4096__USE_BN_ON_LOAD_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused "
        "pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "fp_c1_3_plan_defer_last_128__USE_BN_ON_LOAD_off":
        "pn2_linear pn2_fp_hoist_rows pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad "
        "pn2_linear_wgrad_accumulate pn2_linear_wgrad_accumulate",
    "stack_64_64_rows4096__USE_BN_GRAD_ON_LOAD_off":
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_relu_backward_mode "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_accumulate_xf pn2_bn_relu_backward_mode pn2_linear_dgrad pn2_linear_wgrad",
    "stack_20_32_rows4096__USE_BN_GRAD_ON_LOAD_off":
        "pn2_linear pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_relu_backward_mode "
        "pn2_linear_dgrad_fin pn2_linear_wgrad_accumulate_xf pn2_bn_relu_backward_mode pn2_linear_dgrad pn2_linear_wgrad",
    "sa_c3_32_32_64_rows4096__USE_BN_GRAD_ON_LOAD_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_relu_backward_mode pn2_linear_dgrad_fin pn2_linear_wgrad_accumulate_xf "
        "pn2_bn_relu_backward_mode pn2_linear_dgrad_fin pn2_linear_wgrad_accumulate_xf pn2_bn_relu_backward_mode "
        "pn2_linear_wgrad",
    "sa_c3_64_pooled_first__USE_BN_GRAD_ON_LOAD_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_pool pn2_bn_relu_backward_mode "
        "pn2_linear_wgrad",
    "sa_c3_32_32_64_rows4096__USE_POOLED_BN_REDUCE_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "sa_c3_64_pooled_first__USE_POOLED_BN_REDUCE_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_bn_relu_forward_pool pn2_bn_grad_constants "
        "pn2_linear_wgrad_gx",
    "stack_64_64_rows4096__USE_FUSED_BWD_NARROW_off":
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx",
    "sa_c3_32_32_64_rows4096__USE_FUSED_BWD_NARROW_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_first_layer_bn pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_linear_wgrad_gx",
    "sa_c3_32_32_64_rows4096__USE_SA_FIRST_LAYER_FUSED_off":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats_fin "
        "pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused "
        "pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "sa_c3_32_32_64_rows2048__USE_SA_FIRST_LAYER_FUSED_off":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_wgrad_gx",
    "sa_c3_64_pooled_first__USE_SA_FIRST_LAYER_FUSED_off":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point pn2_sa_group_concat pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_wgrad_gx",
    "sa_c64_64_64_128_plan_rows32768__USE_HOIST_BN_STATS_off":
        "pn2_linear pn2_sa_hoist_rows pn2_bn_relu_forward_deferred pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_pool pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused "
        "pn2_bn_relu_backward_mode pn2_scatter_plan_apply pn2_linear_dgrad pn2_linear_wgrad_accumulate "
        "pn2_linear_wgrad_accumulate",
    "sa_c64_64_64_128_plan_rows4096__USE_HOISTED_TRAIN_off":
        "pn2_sa_group_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_bn_relu_forward_pool "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_bwd_fused pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_scatter_plan_apply",
    "fp_c1_3_plan_defer_last_128__USE_HOISTED_TRAIN_off":
        "pn2_fp_interp_concat pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin "
        "pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_scatter_plan_apply",
    "msg_two_scales_hoisted__USE_HOISTED_MSG_TRAIN_off":
        "pn2_group_point pn2_group_point pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin "
        "pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_group_point pn2_group_point "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_linear_bwd_fused pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_group_point_grad_ws pn2_bn_grad_constants "
        "pn2_linear_bwd_fused pn2_linear_bwd_fused pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_group_point_grad_ws",
    "msg_one_layer_scale_hoisted__USE_HOISTED_MSG_TRAIN_off":
        "pn2_group_point pn2_group_point pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_group_point pn2_group_point "
        "pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode pn2_linear_bn_stats_fin pn2_bn_relu_forward_mode "
        "pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_linear_dgrad_fin pn2_linear_wgrad_gx "
        "pn2_group_point_grad_ws pn2_bn_grad_constants pn2_linear_dgrad_fin pn2_linear_wgrad_gx pn2_group_point_grad_ws",
    "stack_64_64_rows4096__stats_finish_grad_on_load_off":
        "pn2_linear pn2_bn_relu_forward_deferred pn2_linear_bn_stats_xf pn2_bn_relu_forward_mode pn2_bn_relu_backward_mode "
        "pn2_linear_dgrad_bn_grad_stats pn2_linear_wgrad_accumulate_xf pn2_bn_relu_backward_mode pn2_linear_dgrad "
        "pn2_linear_wgrad",
}


def test_every_case_is_pinned():
    assert [c["name"] for c in training_routes.CASES] == list(EXPECTED)


@pytest.mark.parametrize("case", training_routes.CASES, ids=[c["name"] for c in training_routes.CASES])
def test_training_route(pn2, cuda, case):
    tfu = pn2.util.tf_util
    before = {k: getattr(tfu, k) for k in training_routes.SWITCHES}
    calls, _ = training_routes.run_case(pn2, case, cuda, seed=200 + training_routes.CASES.index(case))
    assert [name for name, _ in calls] == EXPECTED[case["name"]].split()
    assert {k: getattr(tfu, k) for k in training_routes.SWITCHES} == before  # every switch restored
