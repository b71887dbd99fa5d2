"""MI355X-native PointNet++ SA/FP stack (drop-in for the tf_ops + util/pointnet_util
path of isl-org/Open3D-PointNet2-Semantic3D).  Importing this package loads
libpn2_hip.so; there is no CPU fallback."""
from . import config  # noqa: F401
from . import _lib  # noqa: F401  (fails loudly if the HIP extension is missing)
from . import tf_ops, util  # noqa: F401
from . import model, runtime, dist, train, dataset, downsample, predict, preprocess  # noqa: F401
from .preprocess import parse_text, read_semantic3d_txt, load_labels, point_cloud_txt_to_pcd  # noqa: F401
from . import scene_io, kitti_predict, render, cluster, plane, neighbors, icp  # noqa: F401
from .cluster import euclidean_clusters, cluster_colors, Clusters, describe_clusters, box_wireframe, Boxes  # noqa: F401
from .neighbors import (radius_neighborhoods, estimate_normals, remove_radius_outlier, normal_colors,  # noqa: F401
                        Neighborhoods)
from .icp import registration_icp, evaluate_registration, transform_points, RegistrationResult  # noqa: F401
from .plane import segment_plane, segment_planes, score_planes, Plane  # noqa: F401
from .scene_io import format_ints, write_labels, write_point_cloud_pcd, read_point_cloud_pcd  # noqa: F401
from .scene_io import write_point_cloud_ply, read_point_cloud_ply, read_point_cloud  # noqa: F401
from .tf_ops.tf_sampling import farthest_point_sample, gather_point, prob_sample  # noqa: F401
from .tf_ops.tf_grouping import query_ball_point, group_point, knn_point, select_top_k  # noqa: F401
from .tf_ops.tf_interpolate import three_nn, three_interpolate, interpolate_label_with_color  # noqa: F401
from .util.pointnet_util import (sample_and_group, sample_and_group_all, pointnet_sa_module,  # noqa: F401
                                 pointnet_sa_module_msg, pointnet_fp_module)

__all__ = ["farthest_point_sample", "gather_point", "query_ball_point", "group_point", "three_nn",
           "three_interpolate", "interpolate_label_with_color", "sample_and_group", "sample_and_group_all", "pointnet_sa_module",
           "pointnet_sa_module_msg", "pointnet_fp_module", "model", "config", "tf_ops", "util"]
