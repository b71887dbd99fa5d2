"""The numpy model of pn2_radius_neighborhoods, written from the rules in include/pn2_abi.h ("Fixed-radius neighbourhoods").  All
pairs in float64 -- no grid, no sort -- so it shares nothing with the kernels but the rules; the covariance and the axes are
describe_ref's (the rules say: those of pn2_cluster_describe with m = count, upright = 0).  The moments are int64 sums of values
the rules bound by 2^60: exact.  The model and the library are compared for equality, bit for bit.  Meant for a few thousand
points (the pair matrix is n^2, and the axes are a Python loop per point).

    out = neighborhoods(points, radius, labels, min_neighbors, viewpoint)      # a Result
"""
import collections

import numpy as np

import describe_ref as D

F = np.float64
CELL_LIMIT = 1 << 21

Result = collections.namedtuple("Result", "count moments normals curvature variance header")


def valid_mask(points, labels=None):
    ok = np.isfinite(np.asarray(points, dtype=np.float32)).all(axis=1)
    if labels is not None:
        ok &= np.asarray(labels) >= 0
    return ok


def lattice_bits(n):
    """Q = min(20, (60 - bitlen(n)) >> 1)"""
    return min(20, (60 - int(n).bit_length()) >> 1)


def lattice(n, radius):
    """-> Q, x, h of a call with n points"""
    Q = lattice_bits(n)
    x = int(np.frexp(F(np.float32(radius)))[1])
    return Q, x, np.ldexp(F(1.0), x - Q)


def status_of(p64, ok, radius):
    """1 when a valid point lies 2^21 or more cells of edge radius * (1 + 2^-20) from the valid points' minimum on an axis"""
    if not ok.any():
        return 0
    cell = F(np.float32(radius)) * (F(1.0) + F(1.0) / F(1048576.0))
    v = p64[ok]
    return int((np.floor((v - v.min(0)) / cell) >= CELL_LIMIT).any())


def neighbour_rows(p64, ok, radius, block=256):
    """yields (i, d) for every valid i in ascending order: d (count,3) float64 = x_j - x_i over its neighbours j"""
    r = F(np.float32(radius))
    r2 = r * r
    n = len(p64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, block):
            b = min(n, a + block)
            d = p64[None, :, :] - p64[a:b, None, :]  # (b-a, n, 3)
            link = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]) <= r2
            link &= ok[a:b, None] & ok[None, :]
            for i in range(a, b):
                if ok[i]:
                    yield i, d[i - a][link[i - a]]


def moments_of(q):
    """q (m,3) int64 -> S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz as Python ints (every sum is below 2^60: int64 is exact)"""
    out = [int(q[:, a].sum()) for a in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append(int((q[:, a] * q[:, b]).sum()))
    return out


def normal_of(a2, p, viewpoint):
    """a2 sign-fixed, then turned towards the viewpoint -> float64 (3,)"""
    nrm = D.fix_sign(np.array(a2, dtype=F))
    if viewpoint is not None:
        v = np.asarray(viewpoint, dtype=F)
        w = ((v[0] - p[0]) * nrm[0] + (v[1] - p[1]) * nrm[1]) + (v[2] - p[2]) * nrm[2]
        if w < 0.0:
            nrm = -nrm
    return nrm


def curvature_of(lam):
    t = (lam[0] + lam[1]) + lam[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = lam[2] / t
    return c if c > 0.0 else F(0.0)


def neighborhoods(points, radius, labels=None, min_neighbors=3, viewpoint=None):
    points = np.asarray(points, dtype=np.float32)
    n = len(points)
    ok = valid_mask(points, labels)
    p64 = points.astype(F)
    count = np.zeros(n, dtype=np.int32)
    moments = np.zeros((n, 9), dtype=np.int64)
    normals = np.full((n, 3), np.nan, dtype=np.float32)
    curvature = np.full(n, np.nan, dtype=np.float32)
    variance = np.full((n, 3), np.nan, dtype=F)
    header = np.zeros(8, dtype=np.int32)
    header[0] = status_of(p64, ok, radius)
    if header[0]:
        return Result(count, moments, normals, curvature, variance, header)
    Q, x, h = lattice(n, radius)
    for i, d in neighbour_rows(p64, ok, radius):
        q = np.rint(d / h).astype(np.int64)
        assert np.abs(q).max() <= 1 << Q
        S = moments_of(q)
        m = len(q)
        count[i], moments[i] = m, S
        if m < min_neighbors:
            continue
        _, A = D.covariance(S, m)
        lam, _, _, a2, _ = D.axes_of(A, 0)
        normals[i] = normal_of(a2, p64[i], viewpoint).astype(np.float32)
        curvature[i] = np.float32(curvature_of(lam))
        variance[i] = lam * (h * h)
    header[1:6] = [ok.sum(), (count >= min_neighbors).sum(), count.max() if n else 0, Q, x]
    return Result(count, moments, normals, curvature, variance, header)
