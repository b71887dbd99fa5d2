"""Device-side scene sampling (mirror of the reference's dataset/ package for the step before the SA/FP stack)."""
from . import semantic_dataset, multi_scene, kitti_dataset  # noqa: F401
from .semantic_dataset import SemanticFileData  # noqa: F401
from .multi_scene import SemanticDataset  # noqa: F401
from .kitti_dataset import KittiFileData, KittiDataset  # noqa: F401
