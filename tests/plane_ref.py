"""numpy model of plane segmentation (include/pn2_abi.h, "Plane segmentation"; csrc/pn2_plane.hip), used by the tests only.

Written from the rules of the header, not from the kernels: float64 arithmetic in exactly the order the header writes, comparisons
as IEEE evaluates them (a NaN is false), the sample ranks from the counter-based stream of tests/dataset_stream_ref.py.  Everything
is evaluated under np.errstate(all="ignore"): overflow and NaN are values here, not warnings."""
import math

import numpy as np

from dataset_stream_ref import draw64, sample_stream

RANK_TAG = 2 ** 45


def valid_mask(points, labels=None):
    ok = np.isfinite(points).all(axis=1)
    return ok if labels is None else ok & (np.asarray(labels) >= 0)


def thr2_of(thr):
    t = np.float64(np.float32(thr))
    return t * t


def normal_sq(planes):
    """nn (T,) of planes (T,6), and which of them are not void"""
    a, b, c = planes[:, 3], planes[:, 4], planes[:, 5]
    with np.errstate(all="ignore"):
        nn = (a * a + b * b) + c * c
        live = np.isfinite(nn) & (nn > 0)
    return nn, live


def _inliers64(p64, ok, plane, thr2):
    """p64 (n,3) float64, ok (n,) bool, one plane (6,) float64"""
    nn, live = normal_sq(plane[None])
    if not live[0]:
        return np.zeros(len(p64), dtype=bool)
    with np.errstate(all="ignore"):
        e = (plane[3] * (p64[:, 0] - plane[0]) + plane[4] * (p64[:, 1] - plane[1])) + plane[5] * (p64[:, 2] - plane[2])
        return ok & (e * e <= thr2 * nn[0])


def inliers(points, plane, thr, labels=None):
    """the mask (n,) of the valid inliers of one plane (6,) float64"""
    return _inliers64(points.astype(np.float64), valid_mask(points, labels), np.asarray(plane, dtype=np.float64), thr2_of(thr))


def score(points, planes, thr, labels=None):
    """pn2_plane_score: counts (T,) int32"""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 6)
    p64, ok, thr2 = points.astype(np.float64), valid_mask(points, labels), thr2_of(thr)
    seen = {}  # rows with the same bits are scored once (many trials over few valid points repeat their planes)
    counts = np.zeros(len(planes), dtype=np.int32)
    for t, pl in enumerate(planes):
        key = pl.tobytes()
        if key not in seen:
            seen[key] = _inliers64(p64, ok, pl, thr2).sum()
        counts[t] = seen[key]
    return counts


def axis_allows(normal, nn, axis, cos2):
    a, b, c = normal
    ax, ay, az = (np.float64(v) for v in axis)
    with np.errstate(all="ignore"):
        dt = (a * ax + b * ay) + c * az
        return bool(dt * dt >= (np.float64(cos2) * nn) * ((ax * ax + ay * ay) + az * az))


def sample_ranks(seed, trials, V):
    """(trials,3) int64: the ranks among the valid points of the three sample points of every trial"""
    h = sample_stream(seed, 0, 0)
    idx = np.arange(3 * trials, dtype=np.uint64) + np.uint64(RANK_TAG)
    return (draw64(h, idx) % np.uint64(V)).astype(np.int64).reshape(trials, 3)


def hypotheses(points, valid_idx, seed, trials, axis=None, cos2=0.0):
    """-> planes (trials,6) float64 (six zeros for a void trial), sample (trials,3) point indices, live (trials,) bool"""
    sample = valid_idx[sample_ranks(seed, trials, len(valid_idx))]
    P = points.astype(np.float64)
    A, B, C = P[sample[:, 0]], P[sample[:, 1]], P[sample[:, 2]]
    with np.errstate(all="ignore"):
        u, v = B - A, C - A
        normal = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                           u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    planes = np.concatenate([A, normal], 1)
    nn, live = normal_sq(planes)
    if axis is not None:
        for t in np.nonzero(live)[0]:
            live[t] = axis_allows(normal[t], nn[t], axis, cos2)
    planes[~live] = 0.0
    return planes, sample, live


def orient(plane6, axis=None):
    """(a,b,c,d) of a non-void plane (6,), oriented by exact negation"""
    x0, y0, z0, a, b, c = (np.float64(v) for v in plane6)
    with np.errstate(all="ignore"):
        d = -((a * x0 + b * y0) + c * z0)
        if axis is not None:
            ax, ay, az = (np.float64(v) for v in axis)
            flip = (a * ax + b * ay) + c * az < 0
        else:
            flip = c < 0 if c != 0 else (b < 0 if b != 0 else a < 0)
    out = np.array([a, b, c, d], dtype=np.float64)
    return -out if flip else out


def ransac(points, thr, trials, seed=0, labels=None, axis=None, cos2=0.0):
    """pn2_plane_ransac -> inlier (n,) uint8, plane (4,) float64, header (8,) int32"""
    n = len(points)
    valid_idx = np.nonzero(valid_mask(points, labels))[0]
    V = len(valid_idx)
    none = np.zeros(n, dtype=np.uint8), np.zeros(4, dtype=np.float64)
    if V < 3:
        return none + (np.array([1, 0, 0, -1, -1, -1, V, 0], dtype=np.int32),)
    planes, sample, live = hypotheses(points, valid_idx, seed, trials, axis, cos2)
    if not live.any():
        return none + (np.array([2, 0, 0, -1, -1, -1, V, 0], dtype=np.int32),)
    counts = score(points, planes, thr, labels)
    t = int(np.argmax(counts))  # the first of the largest
    mask = inliers(points, planes[t], thr, labels)
    header = np.array([0, counts[t], t, sample[t, 0], sample[t, 1], sample[t, 2], V, live.sum()], dtype=np.int32)
    return mask.astype(np.uint8), orient(planes[t], axis), header


def planted(seed=7):
    """the planted case of the tests: a ground of 1800 points (slope 0.02 along x, noise of sigma 0.03) and 1200 points of clutter
    in a cube of 40, 3000 in all, the ground first"""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-20, 20, (1800, 2))
    ground = np.column_stack([xy, 0.02 * xy[:, 0] + rs.normal(0, 0.03, 1800)])
    return np.concatenate([ground, rs.uniform(-20, 20, (1200, 3))]).astype(np.float32)


def cos2_of(max_angle):
    """what the wrapper passes for max_angle in degrees"""
    return math.cos(math.radians(max_angle)) ** 2
