"""Which entry points the inference SA / FP modules reach at the smallest shapes on both sides of every routing threshold
(util/pointnet_util.py: SA_ROUTES, FP_FRONT_ROUTES, DENSE_TAIL_ROUTES).  The cases and the traced call are those of
tools/inference_routes.py; the sequences below are the ones the commit before the route lists launched (its output is
profiles/r09_inference_routes_parent.txt).  Only the entry points are pinned, not the output hashes: a later change of summation
order stays possible, a change of route has to be made here too."""
import pytest

from tools import inference_routes

pytestmark = pytest.mark.gpu

# case -> the pn2_* entry points of one module call, in launch order (a refused call is traced too; an in-place *_ld call is
# recorded under the dense entry point's name, _lib._TRACE_ARGS)
EXPECTED = {
    "sa_32_32_64_c3_dense":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_max_fused",
    "sa_32_32_64_c3_column_blocks":
        "pn2_fps_nested pn2_query_ball_point pn2_query_ball_point pn2_sa_mlp_max_fused",
    "sa_64_64_128_c64_hoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_linear pn2_sa_mlp_fused_pre",
    "sa_64_64_128_c64_unhoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_max_fused",
    "sa_128_128_256_c128":
        "pn2_fps_nested pn2_query_ball_point pn2_linear pn2_sa_mlp_fused_pre pn2_linear",
    "sa_256_256_512_c256_rows4096_hoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_linear pn2_sa_mlp_wide_pre",
    "sa_256_256_512_c256_rows4096_unhoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_wide",
    "sa_256_256_512_c256_rows2048_hoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_group_concat pn2_linear pn2_linear pn2_linear",
    "sa_256_256_512_c256_rows2048_unhoisted":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_group_concat pn2_linear pn2_linear pn2_linear",
    "sa_64_64_128_c64_k64":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_max_fused",
    "sa_64_64_128_c64_k48":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_group_concat pn2_linear pn2_linear pn2_linear",
    "sa_64_64_128_bf16_c64":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_max_fused_bf16",
    "sa_64_64_128_bf16_c8":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_mlp_max_fused",
    "sa_32_32_64_c3_fused_off":
        "pn2_fps_nested pn2_query_ball_point pn2_sa_group_concat pn2_linear pn2_linear pn2_linear",
    "msg_two_scales_c64":
        "pn2_fps_nested pn2_gather_point pn2_query_ball_point_multi pn2_sa_mlp_max_fused pn2_linear pn2_sa_mlp_fused_pre",
    "fp_128x3_c2_128_c1_3_rows65536_hoisted":
        "pn2_linear pn2_fp_mlp_fused_pre",
    "fp_128x3_c2_128_c1_3_rows65536_unhoisted":
        "pn2_fp_mlp_fused pn2_mlp_wide",
    "fp_128x3_c2_128_c1_3_rows65568_hoisted":
        "pn2_linear pn2_fp_mlp_fused_pre",
    "fp_128x3_c2_128_c1_3_rows65568_unhoisted":
        "pn2_fp_mlp_fused pn2_mlp_chain",
    "fp_128x3_c2_128_c1_3_rows65504_hoisted":
        "pn2_fp_interp_concat pn2_mlp_wide",
    "fp_128x3_c2_128_c1_3_rows65504_unhoisted":
        "pn2_fp_interp_concat pn2_mlp_wide",
    "fp_128x3_c2_128_c1_3_rows65536_column_block":
        "pn2_linear pn2_fp_mlp_fused_pre",
    "fp_256x2_c2_256_c1_128_rows4096":
        "pn2_linear pn2_fp_mlp_wide_pre",
    "fp_256x2_c2_256_no_points1_rows4096":
        "pn2_fp_mlp_wide",
    "fp_256x2_c2_256_c1_128_rows4032":
        "pn2_fp_interp_concat pn2_linear pn2_linear",
    "fp_256x2_c2_256_no_points1_rows4032":
        "pn2_fp_interp_concat pn2_linear pn2_linear",
    "fp_128x3_rows65536_chain_off":
        "pn2_fp_interp_concat pn2_mlp_wide",
    "fp_256x2_c1_128_rows4096_wide_off":
        "pn2_fp_interp_concat pn2_linear pn2_linear",
    "fp_128x3_rows65536_fused_fp_off":
        "pn2_fp_interp_concat pn2_mlp_wide",
    "fp_256x2_c1_128_rows4096_fused_fp_off":
        "pn2_fp_interp_concat pn2_mlp_wide",
}


def test_every_case_is_pinned():
    assert [c["name"] for c in inference_routes.CASES] == list(EXPECTED)


@pytest.mark.parametrize("case", inference_routes.CASES, ids=[c["name"] for c in inference_routes.CASES])
def test_inference_route(pn2, cuda, case):
    pu = pn2.util.pointnet_util
    before = {k: getattr(pu, k) for k in case["switches"]}
    calls, _ = inference_routes.run_case(pn2, case, cuda, seed=100 + inference_routes.CASES.index(case))
    assert [name for name, _ in calls] == EXPECTED[case["name"]].split()
    assert {k: getattr(pu, k) for k in case["switches"]} == before  # every switch restored
