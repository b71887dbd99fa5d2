"""Labelled points into objects: Euclidean clustering on the device, where a user of the reference would copy the cloud to the
host and run a KD-tree and a graph library over it.  The kernels are csrc/pn2_cluster.hip; the rules are in include/pn2_abi.h
(pn2_cluster_points) and tests/cluster_ref.py is their numpy model.

    c = euclidean_clusters(points, eps=0.5, labels=dense_labels, classes=[8], min_points=10)   # which points form one car
    c.count, c.ids, c.first, c.size, c.label, c.bbox                                           # how many cars, and where
    img = render.render_colors(points, cluster_colors(c.ids), "top")                           # coloured by instance
    b = describe_clusters(points, c, upright=True)                                             # what each car looks like
    b.centroid, b.axes, b.center, b.extent, b.yaw()                                            # where, which way, how long and wide
    edge_points, owner = box_wireframe(b)                                                      # the boxes, for Renderer.splat

Two points belong to one cluster when a chain of points of their label leads from one to the other in steps of at most eps.
The number of clusters is data-dependent and is read by the host once (the header): the call is eager and refuses a capturing
stream.  Nothing in a result depends on the order in which threads arrive.
"""
import collections
import math

import numpy as np
import torch

from ._lib import launch, ptr, require_cuda, workspace
from .predict import _on_device

# the status word of pn2_cluster_points (include/pn2_abi.h), the convention of downsample.STATUS_NAMES
STATUS_NAMES = {1: "more than 2^21 cells of edge eps on an axis"}

Clusters = collections.namedtuple("Clusters", "ids count first size label bbox")
Clusters.__doc__ = """ids (n,) int32: the cluster of every point, -1 for none; count: the number of clusters (a host int, may be 0);
first, size, label (count,) int32: the lowest point index, the point count and the label (0 without labels) of each cluster, in
ascending order of first; bbox (count,6) float32: min x, y, z then max x, y, z.  Device tensors except count."""


def _device_of(points, labels):
    for a in (points, labels):
        if torch.is_tensor(a):
            require_cuda(a)
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _check_cloud(points, labels, classes):
    """the shape and dtype checks of a (labelled) cloud, before the library is touched -> n, the sorted classes or None"""
    shape = tuple(points.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points: (n,3)")
    n = shape[0]
    if labels is not None:
        if tuple(labels.shape) != (n,):
            raise ValueError("labels: (n,) for points (n,3)")
        kind = labels.dtype
        if (kind.is_floating_point or kind == torch.bool) if torch.is_tensor(labels) else kind.kind not in "iu":
            raise ValueError("labels: integers")
    if classes is not None:
        if labels is None:
            raise ValueError("classes without labels")
        classes = sorted({int(c) for c in classes})
        if any(c < 0 for c in classes):
            raise ValueError("classes: labels >= 0")
    if n >= 2 ** 31:
        raise ValueError("fewer than 2^31 points")
    return n, classes


def _device_cloud(points, labels, classes):
    """-> the device, float32 points and int32 labels (or None) on it, every label outside `classes` turned into -1"""
    dev = _device_of(points, labels)
    points = _on_device(points, torch.float32, dev)
    if labels is not None:
        labels = _on_device(labels, torch.int32, dev)
        if classes is not None:
            labels = torch.where(torch.isin(labels, torch.tensor(classes, dtype=torch.int32, device=dev)), labels,
                                 torch.full_like(labels, -1))
    return dev, points, labels


def euclidean_clusters(points, eps, labels=None, classes=None, min_points=1, max_points=None):
    """points (n,3), labels (n,) integers or None: device tensors or numpy arrays (cast to float32 / int32).  classes: an iterable
    of the labels to cluster -- every other label counts as -1, "no object"; None clusters every label >= 0.  min_points,
    max_points: the sizes of the clusters kept (max_points None or 0: no upper bound).  -> Clusters.
    RuntimeError on a capturing stream; ValueError for a bad argument (before the library is touched) and for a cloud that spans
    more than 2^21 cells of edge eps on an axis (STATUS_NAMES; one host read, of the header)."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("euclidean_clusters is eager (the number of clusters is read by the host): not on a capturing stream")
    try:
        with np.errstate(over="ignore"):  # too large for float32 is inf, refused below
            eps = float(np.float32(eps))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("eps: a number")
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("eps: finite and greater than 0 as float32")
    min_points, max_points = int(min_points), int(max_points or 0)
    if min_points < 1:
        raise ValueError("min_points: at least 1")
    if max_points < 0:
        raise ValueError("max_points: at least 0 (0 or None: no upper bound)")
    if max_points and max_points < min_points:
        raise ValueError("max_points below min_points")
    n, classes = _check_cloud(points, labels, classes)
    dev, points, labels = _device_cloud(points, labels, classes)
    ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
    empty = Clusters(ids, 0, *(torch.empty((0,), dtype=torch.int32, device=dev) for _ in range(3)),
                     torch.empty((0, 6), dtype=torch.float32, device=dev))
    if n == 0:
        return empty  # nothing is launched: the entry point refuses n == 0
    header = torch.zeros((8,), dtype=torch.int32, device=dev)
    ws = workspace("pn2_cluster_workspace_size", dev, n)
    launch("pn2_cluster_points", dev, n, ptr(points), ptr(labels), eps, min_points, max_points, ptr(ids), ptr(header), ptr(ws),
           ws.numel())
    status, count = header[:2].tolist()  # the one host read
    if status:
        raise ValueError("pn2_cluster_points: %s" % STATUS_NAMES[status])
    if count == 0:
        return empty
    first, size, label = (torch.empty((count,), dtype=torch.int32, device=dev) for _ in range(3))
    bbox = torch.empty((count, 6), dtype=torch.float32, device=dev)
    launch("pn2_cluster_stats", dev, n, count, ptr(points), ptr(labels), ptr(ids), ptr(first), ptr(size), ptr(label), ptr(bbox))
    return Clusters(ids, count, first, size, label, bbox)


def cluster_colors(ids):
    """ids (n,) int32 on the device -> (n,3) uint8: one fixed colour of full saturation per id (the hash is in
    include/pn2_abi.h, pn2_cluster_colors), (96,96,96) for -1.  For render.Renderer.image and render.render_colors."""
    require_cuda(ids)
    if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError("ids: (n,) integers")
    ids = ids.to(torch.int32).contiguous()
    n = int(ids.shape[0])
    rgb = torch.empty((n, 3), dtype=torch.uint8, device=ids.device)
    if n:
        launch("pn2_cluster_colors", ids.device, n, ptr(ids), ptr(rgb))
    return rgb


# ---- what each object looks like: moments, principal axes, oriented boxes (csrc/pn2_describe.hip) --------------------------------
class Boxes(collections.namedtuple("Boxes", "size centroid variance axes center extent lo hi moments")):
    """Per cluster, device tensors (the rules are in include/pn2_abi.h, pn2_cluster_describe): size (C,) int64 members (finite
    points of the id); centroid (C,3); variance (C,3) along the axes; axes (C,3,3), row k = the unit axis a_k (a0 the longest
    spread; a right-handed frame); center (C,3) the box centre; extent (C,3) = hi - lo, the box edges along the axes; lo, hi (C,3)
    the members' least and greatest coordinate along each axis, measured from the centroid; moments (C,12) int64, the exact
    integer sums everything else follows from.  float64 except size and moments.  A cluster without members has size 0 and NaNs."""
    __slots__ = ()

    def corners(self):
        """-> (C,8,3) float64: corner j (bits j0 j1 j2) = centroid + sum_k a_k * (hi_k if bit k of j else lo_k).  Plain torch
        ops: a convenience, not part of the exact comparison."""
        bits = torch.tensor([[(j >> k) & 1 for k in range(3)] for j in range(8)], dtype=torch.bool, device=self.lo.device)
        e = torch.where(bits[None], self.hi[:, None, :], self.lo[:, None, :])  # (C,8,3)
        return self.centroid[:, None, :] + e @ self.axes

    def yaw(self):
        """-> (C,) float64: the heading of a0 in the x-y plane, atan2(a0_y, a0_x) (a convenience)"""
        return torch.atan2(self.axes[:, 0, 1], self.axes[:, 0, 0])


def _empty_boxes(dev):
    z3 = torch.empty((0, 3), dtype=torch.float64, device=dev)
    return Boxes(torch.empty((0,), dtype=torch.int64, device=dev), z3, z3.clone(), torch.empty((0, 3, 3), dtype=torch.float64, device=dev),
                 z3.clone(), z3.clone(), z3.clone(), z3.clone(), torch.empty((0, 12), dtype=torch.int64, device=dev))


def _boxes_of(moments, desc):
    lo, hi = desc[:, 15:18], desc[:, 18:21]
    return Boxes(moments[:, 0], desc[:, 0:3], desc[:, 3:6], desc[:, 6:15].reshape(-1, 3, 3), desc[:, 21:24], hi - lo, lo, hi, moments)


def describe_clusters(points, clusters, upright=False):
    """points (n,3): a device tensor or a numpy array (cast to float32).  clusters: a Clusters, or (ids, count) with ids (n,)
    integers and count the number of clusters.  upright: keep a2 = (0,0,1) and turn the box about it only (a vehicle on a road);
    otherwise the three principal axes.  -> Boxes.  count == 0 returns empty tensors without a launch.
    Exact and reproducible: integer moments on a per-cluster lattice, float64 in a fixed association after them.
    RuntimeError on a capturing stream; ValueError for a bad argument, before the library is touched."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("describe_clusters refuses a capturing stream (nothing captures it yet)")
    if isinstance(clusters, Clusters):
        ids, count = clusters.ids, clusters.count
    else:
        try:
            ids, count = clusters
        except (TypeError, ValueError):
            raise ValueError("clusters: a Clusters or (ids, count)")
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)):
        raise ValueError("count: an int")
    count = int(count)
    n, _ = _check_cloud(points, None, None)
    if not (torch.is_tensor(ids) or isinstance(ids, np.ndarray)) or tuple(ids.shape) != (n,):
        raise ValueError("ids: (n,) for points (n,3)")
    if (ids.dtype.is_floating_point or ids.dtype == torch.bool) if torch.is_tensor(ids) else ids.dtype.kind not in "iu":
        raise ValueError("ids: integers")
    if count < 0 or count > n:
        raise ValueError("count: between 0 and the number of points")
    dev = _device_of(points, ids)
    if count == 0:
        return _empty_boxes(dev)
    points = _on_device(points, torch.float32, dev)
    ids = _on_device(ids, torch.int32, dev)
    moments = torch.empty((count, 12), dtype=torch.int64, device=dev)
    desc = torch.empty((count, 24), dtype=torch.float64, device=dev)
    ws = workspace("pn2_cluster_describe_workspace_size", dev, count)
    launch("pn2_cluster_describe", dev, n, count, ptr(points), ptr(ids), 1 if upright else 0, ptr(moments), ptr(desc), ptr(ws),
           ws.numel())
    return _boxes_of(moments, desc)


def box_wireframe(boxes, per_edge=64):
    """boxes: a Boxes.  -> points (C*12*per_edge, 3) float32, owner (C*12*per_edge,) int32: the 12 edges of every box as per_edge
    points each and the cluster each belongs to.  Drawn after the cloud with render.Renderer.splat(points, view, index0=n), with
    cluster_colors(owner) appended to the cloud's colours.  The box of a cluster without members is NaN points: culled."""
    if not isinstance(boxes, Boxes):
        raise ValueError("boxes: a Boxes")
    if isinstance(per_edge, bool) or not isinstance(per_edge, (int, np.integer)) or per_edge < 2:
        raise ValueError("per_edge: an int, at least 2")
    per_edge, count = int(per_edge), int(boxes.size.shape[0])
    if count * 12 * per_edge >= 2 ** 31:
        raise ValueError("fewer than 2^31 wireframe points")
    dev = boxes.size.device
    points = torch.empty((count * 12 * per_edge, 3), dtype=torch.float32, device=dev)
    owner = torch.empty((count * 12 * per_edge,), dtype=torch.int32, device=dev)
    if count:
        require_cuda(boxes.size)
        desc = torch.cat([boxes.centroid, boxes.variance, boxes.axes.reshape(count, 9), boxes.lo, boxes.hi, boxes.center], 1).contiguous()
        launch("pn2_box_wireframe", dev, count, ptr(desc), per_edge, ptr(points), ptr(owner))
    return points, owner
