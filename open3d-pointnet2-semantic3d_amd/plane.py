"""The dominant plane of a cloud on the device: RANSAC plane segmentation, where a user of the reference would copy the frame to
the host for Open3D's segment_plane.  The kernels are csrc/pn2_plane.hip; the rules are in include/pn2_abi.h ("Plane
segmentation") and tests/plane_ref.py is their numpy model.

    ground = segment_plane(points, 0.2, trials=1024, axis=(0, 0, 1), max_angle=15)     # the ground of a LiDAR frame
    ground.model, ground.count, ground.inliers                                         # unit normal and offset, how many, which
    height = ground.distance(points)                                                   # height above ground
    objects = euclidean_clusters(points, 0.5, labels=torch.where(ground.inliers, -1, labels))
    walls = segment_planes(points, 0.05, max_planes=4, min_inliers=500)                # peel plane after plane
    counts = score_planes(points, torch.stack([p.raw for p in walls]), 0.05)           # last frame's planes on this frame

The library decides with float64 comparisons in a fixed order and integers, so a result is the same on every run and equal to
the model's; only `model` and `distance`, which normalise with torch's sqrt and division, are rounded.  One host read per plane
(the header): the calls are eager and refuse a capturing stream.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from ._lib import launch, ptr, workspace
from .cluster import _check_cloud, _device_cloud
from .predict import _on_device

# the status word of pn2_plane_ransac (include/pn2_abi.h)
STATUS_NAMES = {1: "fewer than 3 valid points", 2: "every trial void (repeated or collinear samples, or excluded by the axis)"}
MAX_TRIALS = 2 ** 20
MAX_PLANES = 2 ** 24  # of one pn2_plane_score call


class Plane(collections.namedtuple("Plane", "model raw inliers count sample trial valid status")):
    """model (4,) float64: unit normal and offset (a,b,c,d), a*x + b*y + c*z + d = 0, computed from raw with torch ops; raw (4,)
    float64: the library's exact, unnormalised output; inliers (n,) bool; count: the number of inliers; sample: the three point
    indices the plane was drawn through; trial: the winning trial; valid: the number of valid points; status: 0, or a key of
    STATUS_NAMES -- then count is 0, inliers all False, model and raw zeros, sample (-1,-1,-1).  Device tensors except the ints."""
    __slots__ = ()

    def distance(self, points):
        """points (n,3), a device tensor or a numpy array -> (n,) float64 on the device: the signed distance to the plane, positive
        on the side the normal points to (with axis = (0,0,1): the height above ground)"""
        p = _on_device(points, torch.float64, self.model.device)
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError("points: (n,3)")
        m = self.model
        return ((p[:, 0] * m[0] + p[:, 1] * m[1]) + p[:, 2] * m[2]) + m[3]


def _threshold(distance_threshold):
    try:
        with np.errstate(over="ignore"):  # too large for float32 is inf, refused below
            thr = float(np.float32(distance_threshold))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("distance_threshold: a number")
    if not (math.isfinite(thr) and thr > 0.0):
        raise ValueError("distance_threshold: finite and greater than 0 as float32")
    return thr


def _axis(axis, max_angle):
    """-> (a host array of 3 doubles, cos2) or (None, 0.0)"""
    if axis is None:
        if max_angle is not None:
            raise ValueError("max_angle without axis")
        return None, 0.0
    if max_angle is None:
        raise ValueError("axis without max_angle")
    try:
        axis = [float(v) for v in axis]
        max_angle = float(max_angle)
    except (TypeError, ValueError):
        raise ValueError("axis: three numbers; max_angle: degrees")
    if len(axis) != 3 or not all(math.isfinite(v) for v in axis) or not any(axis):
        raise ValueError("axis: three finite numbers, not all zero")
    if not 0.0 <= max_angle <= 90.0:
        raise ValueError("max_angle: degrees in [0, 90]")
    return (ctypes.c_double * 3)(*axis), math.cos(math.radians(max_angle)) ** 2


def _no_plane(n, dev, status, valid=0):
    zeros = torch.zeros((4,), dtype=torch.float64, device=dev)
    return Plane(zeros, zeros.clone(), torch.zeros((n,), dtype=torch.bool, device=dev), 0, (-1, -1, -1), 0, valid, status)


def _ransac(dev, points, labels, thr, trials, seed, axis, cos2):
    """device points (n,3) float32, labels (n,) int32 or None, n >= 1 -> Plane"""
    n = int(points.shape[0])
    inlier = torch.empty((n,), dtype=torch.uint8, device=dev)
    raw = torch.empty((4,), dtype=torch.float64, device=dev)
    header = torch.empty((8,), dtype=torch.int32, device=dev)
    ws = workspace("pn2_plane_workspace_size", dev, n, trials)
    launch("pn2_plane_ransac", dev, n, ptr(points), ptr(labels), thr, trials, seed, axis, cos2, ptr(inlier), ptr(raw), ptr(header),
           ptr(ws), ws.numel())
    status, count, trial, s0, s1, s2, valid, _ = header.tolist()  # the one host read
    if status:
        return _no_plane(n, dev, status, valid)
    model = raw / torch.sqrt((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2])
    return Plane(model, raw, inlier.bool(), count, (s0, s1, s2), trial, valid, 0)


def _arguments(points, distance_threshold, trials, seed, labels, classes, axis, max_angle):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("plane segmentation is eager (the header is read by the host): not on a capturing stream")
    thr = _threshold(distance_threshold)
    trials, seed = int(trials), int(seed)
    if not 1 <= trials <= MAX_TRIALS:
        raise ValueError("trials: 1 to 2^20")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed: 0 to 2^64 - 1")
    n, classes = _check_cloud(points, labels, classes)
    axis, cos2 = _axis(axis, max_angle)
    return thr, trials, seed, n, classes, axis, cos2


def segment_plane(points, distance_threshold, trials=1024, seed=0, labels=None, classes=None, axis=None, max_angle=None):
    """The plane with the most points within distance_threshold of it, among `trials` planes through three random valid points
    each (the draws depend on seed alone).  points (n,3), labels (n,) integers or None: device tensors or numpy arrays (cast to
    float32 / int32); a point with a non-finite coordinate or a label < 0 takes no part.  classes: the labels that take part
    (every other label counts as -1), as in euclidean_clusters.  axis (3 numbers) with max_angle (degrees, 0 to 90): only planes
    whose normal is within max_angle of the axis or of its opposite; the normal then points along the axis.  -> Plane.
    No plane (fewer than 3 valid points, every trial void) is an answer, not an error: count 0 and a status.  ValueError for a
    bad argument, before the library is touched; RuntimeError on a capturing stream."""
    thr, trials, seed, n, classes, axis, cos2 = _arguments(points, distance_threshold, trials, seed, labels, classes, axis,
                                                          max_angle)
    dev, points, labels = _device_cloud(points, labels, classes)
    if n == 0:
        return _no_plane(0, dev, 1)  # nothing is launched: the entry point refuses n == 0
    return _ransac(dev, points, labels, thr, trials, seed, axis, cos2)


def segment_planes(points, distance_threshold, max_planes, min_inliers, trials=1024, seed=0, labels=None, classes=None, axis=None,
                   max_angle=None):
    """Peels planes off the cloud: after each plane its inliers leave the valid set (their label becomes -1) and the seed advances
    by one.  It stops after max_planes planes, or at the first plane with fewer than min_inliers inliers, which is not returned.
    -> a list of Plane (inliers index `points`).  One host read per plane.  The other arguments as segment_plane."""
    max_planes, min_inliers = int(max_planes), int(min_inliers)
    if max_planes < 1:
        raise ValueError("max_planes: at least 1")
    if min_inliers < 1:
        raise ValueError("min_inliers: at least 1")
    thr, trials, seed, n, classes, axis, cos2 = _arguments(points, distance_threshold, trials, seed, labels, classes, axis,
                                                          max_angle)
    dev, points, labels = _device_cloud(points, labels, classes)
    planes = []
    if n == 0:
        return planes
    if labels is None:
        labels = torch.zeros((n,), dtype=torch.int32, device=dev)
    for k in range(max_planes):
        plane = _ransac(dev, points, labels, thr, trials, (seed + k) % 2 ** 64, axis, cos2)
        if plane.count < min_inliers:
            break
        planes.append(plane)
        labels = torch.where(plane.inliers, torch.full_like(labels, -1), labels)
    return planes


def score_planes(points, planes, distance_threshold, labels=None):
    """How many valid points of the cloud lie within distance_threshold of each plane -> (T,) int32 on the device; 0 for a void
    plane (a zero or non-finite normal).  planes: (T,6) float64 rows (x0,y0,z0, a,b,c), a point on the plane and a normal of any
    length, or (T,4) rows (a,b,c,d) such as Plane.raw or Plane.model.  A (T,4) row is converted in torch, in float64, to the
    point of the plane nearest the origin, (x0,y0,z0) = (a,b,c) * (-d / ((a*a + b*b) + c*c)): that division rounds, so pass (T,6)
    rows where the count must equal the one segment_plane reported.  No host read."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("score_planes refuses a capturing stream")
    thr = _threshold(distance_threshold)
    n, _ = _check_cloud(points, labels, None)
    shape = tuple(getattr(planes, "shape", ()))  # (anything without a shape, a list of rows say, is refused like a wrong one)
    if len(shape) != 2 or shape[1] not in (4, 6):
        raise ValueError("planes: a (T,6) array or tensor of rows (x0,y0,z0,a,b,c), or (T,4) of rows (a,b,c,d)")
    if shape[0] > MAX_PLANES:
        raise ValueError("planes: 2^24 rows at the most in one call")
    dev, points, labels = _device_cloud(points, labels, None)
    planes = _on_device(planes, torch.float64, dev)
    if shape[1] == 4:
        normal, d = planes[:, :3], planes[:, 3:]
        nn = (normal[:, 0:1] * normal[:, 0:1] + normal[:, 1:2] * normal[:, 1:2]) + normal[:, 2:3] * normal[:, 2:3]
        planes = torch.cat([normal * (-d / nn), normal], 1).contiguous()
    counts = torch.zeros((shape[0],), dtype=torch.int32, device=dev)
    if n and shape[0]:
        launch("pn2_plane_score", dev, n, ptr(points), ptr(labels), shape[0], ptr(planes), thr, ptr(counts))
    return counts
