from . import tf_util, pointnet_util, metric  # noqa: F401
