"""How one cloud lies on another: rigid registration by iterative closest point on the device -- point-to-point and
point-to-plane -- where a user of the reference would copy both clouds to the host and build a KD-tree (Open3D's
registration_icp, evaluate_registration and PointCloud.transform).  The kernels are csrc/pn2_icp.hip; the rules are in
include/pn2_abi.h ("Rigid registration (ICP)") and tests/icp_ref.py is their numpy model.

    reg = registration_icp(frame_k, frame_k_minus_1, 0.5)                          # reg.transformation: (4,4) float64
    reg = registration_icp(src, tgt, 0.5, estimation="point_to_plane", target_normals=estimate_normals(tgt, 0.8))
    ev = evaluate_registration(src, tgt, 0.5, init=reg.transformation)             # fitness and inlier rmse of a given pose
    merged = torch.cat([tgt, transform_points(src, reg.transformation)])

The whole loop runs inside one call without a host synchronisation; the host reads one small buffer at the end.  Every result is
reproducible bit for bit: float64 sums in one fixed tree over the source's order (so a permuted source may differ in the last
bits -- the one place where this module departs from the integer sums of its neighbours).  The calls are eager and refuse a
capturing stream."""
import collections
import ctypes
import math

import numpy as np
import torch

from ._lib import launch, ptr, workspace
from .cluster import _check_cloud, _device_cloud, _on_device
from .neighbors import _radius

# the status word of pn2_icp (include/pn2_abi.h), the convention of cluster.STATUS_NAMES
STATUS_NAMES = {1: "more than 2^21 cells of edge max_correspondence_distance on an axis of the target",
                2: "too few correspondences, or they do not determine the motion"}
ESTIMATIONS = {"point_to_point": 0, "point_to_plane": 1}

RegistrationResult = collections.namedtuple("RegistrationResult",
                                            "transformation fitness inlier_rmse correspondence iterations converged status trace")
RegistrationResult.__doc__ = """transformation (4,4) float64 numpy: source -> target; fitness: the share of the valid source points
that have a partner; inlier_rmse over those pairs; correspondence (ns,) int32 on the device: the partner's target index or -1;
iterations: the updates applied; converged: the criterion stopped the loop; status: 0, or a key of STATUS_NAMES (1: nothing was
matched, 2: the transformation is the last one that could be formed); trace: None, or (iterations + 1, 20) float64 numpy, row k
= (pairs, fitness, rmse, 0, T_k row-major).  Host values except correspondence."""


def _matrix(T, name):
    """-> 16 host doubles, row-major, or None"""
    if T is None:
        return None
    try:
        if torch.is_tensor(T):
            T = T.detach().cpu().numpy()
        a = np.asarray(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: a 4x4 matrix" % name)
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError("%s: a finite 4x4 matrix" % name)
    return (ctypes.c_double * 16)(*a.reshape(-1).tolist())


def _tolerance(v, name):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s: a number" % name)
    if not v >= 0.0:
        raise ValueError("%s: at least 0" % name)
    return v


def registration_icp(source, target, max_correspondence_distance, init=None, estimation="point_to_point", target_normals=None,
                     max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, source_labels=None, target_labels=None,
                     classes=None, trace=False):
    """source (ns,3), target (nt,3), the labels (n,) integers or None, target_normals (nt,3) or None: device tensors or numpy
    arrays (cast to float32 / int32).  init: a 4x4 (None: the identity).  estimation: "point_to_point" or "point_to_plane" (needs
    target_normals, e.g. neighbors.estimate_normals(target, radius); a target point with a NaN normal takes no part).  classes: an
    iterable of the labels that take part, on both sides -- static classes only, say; every other label becomes -1.  The loop stops
    after max_iteration updates or when fitness and rmse both change by less than the two tolerances (Open3D's criterion).
    -> RegistrationResult.  RuntimeError on a capturing stream; ValueError for a bad argument, before the library is touched.
    One host read, of the result and the header in one buffer (and of the trace when asked for)."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("registration_icp is eager (the result is read by the host): not on a capturing stream")
    try:
        radius = _radius(max_correspondence_distance)
    except ValueError as e:
        raise ValueError(str(e).replace("radius", "max_correspondence_distance"))
    if estimation not in ESTIMATIONS:
        raise ValueError("estimation: one of %s" % sorted(ESTIMATIONS))
    est = ESTIMATIONS[estimation]
    if isinstance(max_iteration, bool) or not isinstance(max_iteration, (int, np.integer)) or max_iteration < 0 or max_iteration >= 2 ** 20:
        raise ValueError("max_iteration: an int, 0 <= max_iteration < 2^20")
    max_iteration = int(max_iteration)
    relative_fitness = _tolerance(relative_fitness, "relative_fitness")
    relative_rmse = _tolerance(relative_rmse, "relative_rmse")
    T0 = _matrix(init, "init")
    if (source_labels is None) != (target_labels is None) and classes is not None:
        raise ValueError("classes: needs source_labels and target_labels")
    ns, classes = _check_cloud(source, source_labels, classes)
    nt, _ = _check_cloud(target, target_labels, classes)
    if est and target_normals is None:
        raise ValueError("target_normals: needed for point_to_plane")
    if target_normals is not None and tuple(target_normals.shape) != (nt, 3):
        raise ValueError("target_normals: (nt,3) for target (nt,3)")
    dev, source, source_labels = _device_cloud(source, source_labels, classes)
    with torch.cuda.device(dev):  # (a host array of the target goes where the source is)
        tdev, target, target_labels = _device_cloud(target, target_labels, classes)
    if tdev != dev:
        raise ValueError("source and target: on one device")
    normals = None if target_normals is None else _on_device(target_normals, torch.float32, dev)
    corr = torch.full((ns,), -1, dtype=torch.int32, device=dev)
    eye = np.eye(4) if T0 is None else np.array(list(T0), dtype=np.float64).reshape(4, 4)
    if ns == 0 or nt == 0:  # nothing is launched: the entry point refuses an empty cloud
        return RegistrationResult(eye, 0.0, 0.0, corr, 0, False, 0, np.zeros((1, 20)) if trace else None)
    # result (20 doubles) and header (8 int32) carved from one buffer: one copy to the host
    out = torch.zeros((24,), dtype=torch.float64, device=dev)
    rows = torch.empty((max_iteration + 1, 20), dtype=torch.float64, device=dev) if trace else None
    ws = workspace("pn2_icp_workspace_size", dev, ns, nt, max_iteration)
    launch("pn2_icp", dev, ns, ptr(source), ptr(source_labels), nt, ptr(target), ptr(target_labels), ptr(normals), radius, est, T0,
           max_iteration, relative_fitness, relative_rmse, ptr(corr), ptr(out), ptr(rows), ptr(out, 160), ptr(ws), ws.numel())
    host = out.cpu().numpy()  # the one host read
    h = host[20:].view(np.int32)
    status, updates = int(h[0]), int(h[4])
    return RegistrationResult(host[:16].reshape(4, 4).copy(), float(host[16]), float(host[17]), corr, updates, bool(h[5]), status,
                              rows[:updates + 1].cpu().numpy() if trace else None)


def evaluate_registration(source, target, max_correspondence_distance, init=None, source_labels=None, target_labels=None,
                          classes=None):
    """Open3D's evaluate_registration: fitness, inlier rmse and correspondences of `init` as it stands: registration_icp with
    max_iteration = 0 -> RegistrationResult (transformation = init)."""
    return registration_icp(source, target, max_correspondence_distance, init=init, max_iteration=0, source_labels=source_labels,
                            target_labels=target_labels, classes=classes)


def transform_points(points, transformation):
    """points (n,3) under the 4x4 `transformation` -> (n,3) float32 on the device: per axis float64, rounded to float32 once (the
    rule registration_icp matches under); a row with a non-finite coordinate is copied as it is.  One launch, no host read."""
    T = _matrix(transformation, "transformation")
    if T is None:
        raise ValueError("transformation: a finite 4x4 matrix")
    n, _ = _check_cloud(points, None, None)
    dev, points, _ = _device_cloud(points, None, None)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        launch("pn2_transform_points", dev, n, ptr(points), T, ptr(out))
    return out


def compose(*transformations):
    """the product of 4x4 matrices, the first applied LAST (compose(A, B) @ x = A @ (B @ x)) -> (4,4) float64 numpy"""
    out = np.eye(4)
    for T in transformations:
        out = out @ np.asarray(T.detach().cpu().numpy() if torch.is_tensor(T) else T, dtype=np.float64).reshape(4, 4)
    return out


def rigid_error(T, truth):
    """-> (angle in degrees, distance) between two rigid 4x4 transformations: of the rotation and translation of T @ inv(truth)"""
    E = np.asarray(T, dtype=np.float64) @ np.linalg.inv(np.asarray(truth, dtype=np.float64))
    cos = min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))
    return math.degrees(math.acos(cos)), float(np.linalg.norm(E[:3, 3]))
