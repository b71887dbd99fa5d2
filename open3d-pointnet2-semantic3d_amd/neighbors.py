"""What lies around each point: fixed-radius neighbourhoods on the device -- how many points, which way the surface faces, how
flat it is -- where a user of the reference would copy the cloud to the host and build a KD-tree (Open3D's estimate_normals with
KDTreeSearchParamRadius, remove_radius_outlier).  The kernels are csrc/pn2_neighbors.hip; the rules are in include/pn2_abi.h
("Fixed-radius neighbourhoods") and tests/neighbors_ref.py is their numpy model.

    nb = radius_neighborhoods(points, 0.5, viewpoint=(0, 0, 0))           # count, normals, curvature per point
    keep, mask = remove_radius_outlier(points, nb_points=5, radius=0.5)   # stray returns out, before objects_for_frame
    img = render.render_colors(points, normal_colors(nb.normals), "top")  # something to shade with

A point's neighbours are the valid points within `radius` of it, the point itself included.  Every result is exact and
reproducible: a float64 distance test, integer moments on one lattice per call, float64 in a fixed association after them.
The calls are eager and refuse a capturing stream."""
import collections
import ctypes
import math

import numpy as np
import torch

from ._lib import launch, ptr, workspace
from .cluster import _check_cloud, _device_cloud

# the status word of pn2_radius_neighborhoods (include/pn2_abi.h), the convention of cluster.STATUS_NAMES
STATUS_NAMES = {1: "more than 2^21 cells of edge radius on an axis"}
GREY = (96, 96, 96)

Neighborhoods = collections.namedtuple("Neighborhoods", "count normals curvature variance moments lattice valid status")
Neighborhoods.__doc__ = """count (n,) int32: the neighbours of every point, itself included, 0 for an invalid point; normals (n,3)
float32: unit normals, NaN where count < min_neighbors; curvature (n,) float32: the surface variation lambda_2 / (lambda_0 +
lambda_1 + lambda_2), 0 on a plane, at most 1/3; variance (n,3) float64 along the principal axes, or None; moments (n,9) int64:
the exact integer sums everything else follows from, or None; lattice: (Q, x), the moments' unit is 2^(x-Q); valid: the number
of valid points; status: 0, or a key of STATUS_NAMES (then every count is 0 and the rest NaN).  Device tensors except the last
three, which are host values."""


def _radius(radius):
    try:
        with np.errstate(over="ignore"):  # too large for float32 is inf, refused below
            radius = float(np.float32(radius))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("radius: a number")
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("radius: finite and greater than 0 as float32")
    return radius


def _at_least_one(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError("%s: an int, at least 1" % name)
    return int(value)


def _viewpoint(viewpoint):
    if viewpoint is None:
        return None
    try:
        v = [float(c) for c in viewpoint]
    except (TypeError, ValueError):
        raise ValueError("viewpoint: three numbers")
    if len(v) != 3 or not all(math.isfinite(c) for c in v):
        raise ValueError("viewpoint: three finite numbers")
    return (ctypes.c_double * 3)(*v)


def radius_neighborhoods(points, radius, labels=None, classes=None, min_neighbors=3, viewpoint=None, moments=False, variance=False):
    """points (n,3), labels (n,) integers or None: device tensors or numpy arrays (cast to float32 / int32).  classes: an iterable
    of the labels that count -- every other label becomes -1, an invalid point; None keeps every label >= 0.  min_neighbors: the
    fewest neighbours (the point included) for a normal.  viewpoint: three numbers; every normal then points to its side (a
    sensor at the origin: (0, 0, 0)).  moments, variance: return these as well.  -> Neighborhoods.
    RuntimeError on a capturing stream; ValueError for a bad argument, before the library is touched.  One host read, of the
    32-byte header."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("radius_neighborhoods is eager (the header is read by the host): not on a capturing stream")
    radius = _radius(radius)
    min_neighbors = _at_least_one(min_neighbors, "min_neighbors")
    view = _viewpoint(viewpoint)
    n, classes = _check_cloud(points, labels, classes)
    dev, points, labels = _device_cloud(points, labels, classes)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty((n,), dtype=torch.float32, device=dev)
    var = torch.empty((n, 3), dtype=torch.float64, device=dev) if variance else None
    mom = torch.empty((n, 9), dtype=torch.int64, device=dev) if moments else None
    if n == 0:
        return Neighborhoods(count, normals, curvature, var, mom, (0, 0), 0, 0)  # nothing is launched: the entry point refuses n == 0
    header = torch.zeros((8,), dtype=torch.int32, device=dev)
    ws = workspace("pn2_radius_workspace_size", dev, n)
    launch("pn2_radius_neighborhoods", dev, n, ptr(points), ptr(labels), radius, min_neighbors, view, ptr(count), ptr(mom),
           ptr(normals), ptr(curvature), ptr(var), ptr(header), ptr(ws), ws.numel())
    h = header.tolist()  # the one host read
    return Neighborhoods(count, normals, curvature, var, mom, (h[4], h[5]), h[1], h[0])


def _ok(nb, what):
    if nb.status:
        raise ValueError("%s: %s" % (what, STATUS_NAMES[nb.status]))
    return nb


def estimate_normals(points, radius, viewpoint=None, min_neighbors=3):
    """-> (n,3) float32 on the device: the unit normal of the surface at every point, from the points within `radius` of it; NaN
    where fewer than min_neighbors lie there.  viewpoint: see radius_neighborhoods.  ValueError for a cloud that spans more than
    2^21 cells of edge radius on an axis (STATUS_NAMES)."""
    return _ok(radius_neighborhoods(points, radius, min_neighbors=min_neighbors, viewpoint=viewpoint), "estimate_normals").normals


def select_by_count(count, nb_points):
    """count (n,) integers -> (indices, mask): the points with count >= nb_points, in ascending order (int64), and as (n,) bool.
    Plain torch ops."""
    mask = count >= nb_points
    return torch.nonzero(mask).reshape(-1), mask


def remove_radius_outlier(points, nb_points, radius, labels=None):
    """Open3D's remove_radius_outlier: -> (indices, mask) of the valid points with at least nb_points points within `radius` of
    them, the point itself counted, as in Open3D; indices (k,) int64 ascending, mask (n,) bool, on the device."""
    nb_points = _at_least_one(nb_points, "nb_points")
    return select_by_count(_ok(radius_neighborhoods(points, radius, labels=labels, min_neighbors=nb_points),
                               "remove_radius_outlier").count, nb_points)


def normal_colors(normals):
    """normals (n,3) floating point -> (n,3) uint8: rint((n * 0.5 + 0.5) * 255) per component, (96,96,96) for a row with a NaN.
    Plain torch ops, for render.Renderer.image and render.render_colors."""
    if not torch.is_tensor(normals) or normals.dim() != 2 or normals.shape[1] != 3 or not normals.dtype.is_floating_point:
        raise ValueError("normals: a (n,3) floating-point tensor")
    bad = torch.isnan(normals).any(1, keepdim=True)
    rgb = torch.round((torch.where(bad, torch.zeros_like(normals), normals) * 0.5 + 0.5) * 255.0).clamp(0, 255).to(torch.uint8)
    return torch.where(bad, torch.tensor(GREY, dtype=torch.uint8, device=normals.device), rgb)
