from . import tf_util, pointnet_util, metric, provider  # noqa: F401
