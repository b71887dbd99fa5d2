"""A numpy model of pn2_scene_ingest (include/pn2_abi.h, csrc/pn2_store.hip): one scene of the SemanticDataset store --
stable argsort by x, the casts, the z range, the label histogram, the statuses.  Needs neither torch nor the library."""
import numpy as np


def ingest(points, colors=None, labels=None):
    """points (n,3) float64, colors (n,3) float64 or None, labels (n,) int32 or None ->
    dict(status, perm int32, points float64, colors float32 or None, labels uint8, zrange (2,) float64, hist (9,) int64).
    With a non-zero status only `status` is specified (the others are returned as the rule would give them, for curiosity)."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    lab = np.zeros(n, dtype=np.int32) if labels is None else np.asarray(labels).astype(np.int32)
    status = 0
    if lab.size and (lab.min() < 0 or lab.max() > 255):
        status = 2
    if not np.isfinite(points).all():
        status = 1  # both: 1
    # np.argsort compares -0.0 == +0.0, and kind="stable" keeps equal keys in input order
    perm = np.argsort(points[:, 0], kind="stable").astype(np.int32)
    out = dict(status=status, perm=perm, points=np.ascontiguousarray(points[perm]))
    out["colors"] = None if colors is None else np.ascontiguousarray(
        np.asarray(colors, dtype=np.float64).reshape(-1, 3)[perm].astype(np.float32))
    out["labels"] = lab[perm].astype(np.uint8)
    z = points[:, 2]
    with np.errstate(invalid="ignore"):
        zr = np.array([z.min(), z.max()], dtype=np.float64)
    # the one case numpy leaves to the order of the rows: among zeros the minimum is -0.0 if there is one, the maximum +0.0
    zeros = z[z == 0.0]
    if zr[0] == 0.0:
        zr[0] = -0.0 if np.signbit(zeros).any() else 0.0
    if zr[1] == 0.0:
        zr[1] = 0.0 if (~np.signbit(zeros)).any() else -0.0
    out["zrange"] = zr
    out["hist"] = np.histogram(lab, range(10))[0].astype(np.int64)
    return out
