"""The numpy model of pn2_icp and pn2_transform_points, written from the rules in include/pn2_abi.h ("Rigid registration (ICP)").
The partner search is all pairs in float64 -- no grid, no sort -- so it shares nothing with the kernels but the rules; the sums
are the header's tree (xor butterflies of 64, four waves, workgroups in ascending order), the Jacobi sweeps, the Cholesky and
the 4x4 product are in the header's association.  The model and the library are compared for equality, bit for bit.  Meant for
a few hundred points (the pair matrix is ns x nt).

    out = icp(source, target, max_distance, estimation=0, init=None, max_iteration=30, ...)      # a Result
"""
import collections

import numpy as np

import describe_ref as D

F = np.float64
CELL_LIMIT = 1 << 21
WAVE, BLOCK = 64, 256
NV = (17, 29)  # sums of a point-to-point / point-to-plane evaluation

Result = collections.namedtuple("Result", "correspondence result trace header")


def valid_mask(points, labels=None, normals=None):
    ok = np.isfinite(np.asarray(points, dtype=np.float32)).all(axis=1)
    if labels is not None:
        ok &= np.asarray(labels) >= 0
    if normals is not None:
        ok &= np.isfinite(np.asarray(normals, dtype=np.float32)).all(axis=1)
    return ok


def transform_rows(points, T):
    """TRANSFORMED SOURCE POINT of every row, whether valid or not -> (n,3) float32"""
    p = np.asarray(points, dtype=np.float32).astype(F)
    T = np.asarray(T, dtype=F).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [(((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]).astype(np.float32) for a in range(3)]
    return np.stack(cols, 1)


def transform_points(points, T):
    """pn2_transform_points: invalid rows pass through as they are"""
    points = np.asarray(points, dtype=np.float32)
    ok = np.isfinite(points).all(axis=1)
    out = points.copy()
    out[ok] = transform_rows(points[ok], T)
    return out


def grid_status(t64, t_ok, max_distance):
    """1 when a valid target point lies 2^21 or more cells of edge r * (1 + 2^-20) from the valid points' minimum on an axis"""
    if not t_ok.any():
        return 0
    cell = F(np.float32(max_distance)) * (F(1.0) + F(1.0) / F(1048576.0))
    v = t64[t_ok]
    return int((np.floor((v - v.min(0)) / cell) >= CELL_LIMIT).any())


def partners(sp, s_ok, t64, t_ok, max_distance):
    """sp (ns,3) float32 transformed source -> (index (ns,) int32, d2 (ns,) float64): the PARTNER rule by brute force"""
    r = F(np.float32(max_distance))
    r2 = r * r
    s64 = sp.astype(F)
    ns = len(sp)
    index = np.full(ns, -1, dtype=np.int32)
    best = np.zeros(ns, dtype=F)
    if not t_ok.any():
        return index, best
    with np.errstate(invalid="ignore", over="ignore"):
        d = t64[None, :, :] - s64[:, None, :]  # (ns, nt, 3)
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        d2 = np.where(t_ok[None, :] & (d2 <= r2), d2, np.inf)
    at = np.argmin(d2, axis=1)  # the first of equal minima: the lowest target index
    dmin = d2[np.arange(ns), at]
    has = s_ok & np.isfinite(sp).all(axis=1) & (dmin <= r2)
    index[has] = at[has]
    best[has] = dmin[has]
    return index, best


def lane_rows(est, sp, index, d2, t64, normals, o):
    """(ns, NV) float64: every lane's row of the sums, +0.0 without a partner"""
    ns = len(sp)
    rows = np.zeros((ns, NV[est]), dtype=F)
    has = index >= 0
    if not has.any():
        return rows
    p = sp[has].astype(F) - o
    t = t64[index[has]]
    v = np.zeros((int(has.sum()), NV[est]), dtype=F)
    v[:, 0] = 1.0
    v[:, 1] = d2[has]
    if est == 0:
        u = t - o
        v[:, 2:5] = p
        v[:, 5:8] = u
        for a in range(3):
            for b in range(3):
                v[:, 8 + 3 * a + b] = p[:, a] * u[:, b]
    else:
        n = np.asarray(normals, dtype=np.float32)[index[has]].astype(F)
        e = sp[has].astype(F) - t
        rho = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        J = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2]]
        at = 2
        for a in range(6):
            for b in range(a, 6):
                v[:, at] = J[a] * J[b]
                at += 1
        for a in range(6):
            v[:, 23 + a] = J[a] * rho
    rows[has] = v
    return rows


def tree_sum(rows):
    """SUMS: (ns, nv) lane rows -> (nv,): butterflies inside each wave of 64, ((w0 + w1) + w2) + w3 per workgroup of 256, the
    workgroups added to 0.0 in ascending order"""
    ns, nv = rows.shape
    blocks = (ns + BLOCK - 1) // BLOCK
    v = np.zeros((blocks * BLOCK, nv), dtype=F)
    v[:ns] = rows
    v = v.reshape(blocks, BLOCK // WAVE, WAVE, nv)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o, :]
    w = v[:, :, 0, :]
    g = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    total = np.zeros(nv, dtype=F)
    for b in range(blocks):
        total = total + g[b]
    return total


def rotate4(A, V, p, r):
    """one Jacobi rotation on the pair (p, r) of the full symmetric A, in place: describe_ref.rotate's formula, its third-index
    step applied to both other indices"""
    apr = A[p, r]
    if apr == 0.0:
        return
    with np.errstate(over="ignore"):
        theta = (A[r, r] - A[p, p]) / (F(2.0) * apr)
        sigma = F(1.0) if theta >= 0.0 else F(-1.0)
        t = sigma / (np.abs(theta) + np.sqrt(theta * theta + F(1.0)))
    c = F(1.0) / np.sqrt(t * t + F(1.0))
    s = t * c
    A[p, p] = A[p, p] - t * apr
    A[r, r] = A[r, r] + t * apr
    A[p, r] = A[r, p] = F(0.0)
    for k in range(4):
        if k in (p, r):
            continue
        akp, akr = A[k, p], A[k, r]
        A[k, p] = A[p, k] = c * akp - s * akr
        A[k, r] = A[r, k] = s * akp + c * akr
    for i in range(4):
        vp, vr = V[i, p], V[i, r]
        V[i, p] = c * vp - s * vr
        V[i, r] = s * vp + c * vr


def largest_eigenvector(N):
    """ten cyclic sweeps from V = identity -> the column of V under the largest diagonal entry (the first among equals), and A
    after the sweeps"""
    A = np.array(N, dtype=F)
    V = np.eye(4, dtype=F)
    for _ in range(10):
        for p in range(3):
            for r in range(p + 1, 4):
                rotate4(A, V, p, r)
    at = 0
    for j in range(1, 4):
        if A[j, j] > A[at, at]:
            at = j
    return V[:, at].copy(), A


def rotation_of(w, x, y, z):
    w, x, y, z = F(w), F(x), F(y), F(z)
    nn = ((w * w + x * x) + y * y) + z * z
    two = F(2.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.array([[(((w * w + x * x) - y * y) - z * z) / nn, (two * (x * y - w * z)) / nn, (two * (x * z + w * y)) / nn],
                         [(two * (x * y + w * z)) / nn, (((w * w - x * x) + y * y) - z * z) / nn, (two * (y * z - w * x)) / nn],
                         [(two * (x * z - w * y)) / nn, (two * (y * z + w * x)) / nn, (((w * w - x * x) - y * y) + z * z) / nn]],
                        dtype=F)


def solve_point(S, o):
    """POINT-TO-POINT: the summed row (m >= 3) -> R (3,3), t (3,)"""
    m = S[0]
    pm, um = S[2:5] / m, S[5:8] / m
    M = np.array([[S[8 + 3 * a + b] / m - pm[a] * um[b] for b in range(3)] for a in range(3)], dtype=F)
    N = np.zeros((4, 4), dtype=F)
    N[0, 0] = (M[0, 0] + M[1, 1]) + M[2, 2]
    N[1, 1] = (M[0, 0] - M[1, 1]) - M[2, 2]
    N[2, 2] = (M[1, 1] - M[0, 0]) - M[2, 2]
    N[3, 3] = (M[2, 2] - M[0, 0]) - M[1, 1]
    N[0, 1] = N[1, 0] = M[1, 2] - M[2, 1]
    N[0, 2] = N[2, 0] = M[2, 0] - M[0, 2]
    N[0, 3] = N[3, 0] = M[0, 1] - M[1, 0]
    N[1, 2] = N[2, 1] = M[0, 1] + M[1, 0]
    N[1, 3] = N[3, 1] = M[2, 0] + M[0, 2]
    N[2, 3] = N[3, 2] = M[1, 2] + M[2, 1]
    q, _ = largest_eigenvector(N)
    R = rotation_of(q[0], q[1], q[2], q[3])
    c = pm + o
    t = np.array([(um[a] + o[a]) - ((R[a, 0] * c[0] + R[a, 1] * c[1]) + R[a, 2] * c[2]) for a in range(3)], dtype=F)
    return R, t


def cholesky_solve(A, g):
    """A x = -g by the header's Cholesky -> x (6,), or None for a pivot that is not > 0"""
    n = len(g)
    L = np.zeros((n, n), dtype=F)
    y = np.zeros(n, dtype=F)
    x = np.zeros(n, dtype=F)
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    for i in range(n):
        v = -g[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = v - L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x


def plane_system(S):
    A = np.zeros((6, 6), dtype=F)
    at = 2
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = S[at]
            at += 1
    return A, np.array(S[23:29], dtype=F)


def solve_plane(S, o):
    """POINT-TO-PLANE: the summed row (m >= 6) -> (R, t) or None"""
    A, g = plane_system(S)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = cholesky_solve(A, g)
    if x is None:
        return None
    R = rotation_of(F(1.0), x[0] / F(2.0), x[1] / F(2.0), x[2] / F(2.0))
    t = np.array([(o[a] + x[3 + a]) - ((R[a, 0] * o[0] + R[a, 1] * o[1]) + R[a, 2] * o[2]) for a in range(3)], dtype=F)
    return R, t


def compose(R, t, T):
    """T_(k+1) = U * T_k: rows 0..2 in the header's association, row 3 kept"""
    out = T.copy()
    for a in range(3):
        for b in range(4):
            out[a, b] = ((R[a, 0] * T[0, b] + R[a, 1] * T[1, b]) + R[a, 2] * T[2, b]) + t[a] * T[3, b]
    return out


def icp(source, target, max_distance, estimation=0, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
        source_labels=None, target_labels=None, target_normals=None):
    source = np.asarray(source, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    ns = len(source)
    s_ok = valid_mask(source, source_labels)
    t_ok = valid_mask(target, target_labels, target_normals if estimation else None)
    t64 = target.astype(F)
    T = np.eye(4, dtype=F) if init is None else np.array(init, dtype=F).reshape(4, 4)
    trace = np.zeros((max_iteration + 1, 20), dtype=F)
    result = np.zeros(20, dtype=F)
    header = np.zeros(8, dtype=np.int32)
    status = grid_status(t64, t_ok, max_distance)
    o = np.array([D.key_min(t64[t_ok, a]) for a in range(3)], dtype=F) if t_ok.any() else np.full(3, np.nan)
    nvs = int(s_ok.sum())
    prev = None
    k = 0
    while True:
        sp = transform_rows(source, T)
        if status == 1:
            index, d2 = np.full(ns, -1, dtype=np.int32), np.zeros(ns, dtype=F)
        else:
            index, d2 = partners(sp, s_ok, t64, t_ok, max_distance)
        S = tree_sum(lane_rows(estimation, sp, index, d2, t64, target_normals, o))
        m = S[0]
        fitness = m / F(nvs) if nvs > 0 else F(0.0)
        rmse = np.sqrt(S[1] / m) if m > 0 else F(0.0)
        trace[k, :4] = [m, fitness, rmse, 0.0]
        trace[k, 4:] = T.reshape(-1)
        converged = 0
        stop = status != 0
        if not stop and k >= 1 and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            converged, stop = 1, True
        if not stop and k == max_iteration:
            stop = True
        if not stop:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                if estimation == 0:
                    update = solve_point(S, o) if m >= 3 else None
                else:
                    update = solve_plane(S, o) if m >= 6 else None
                if update is None:
                    status, stop = 2, True
                else:
                    T = compose(update[0], update[1], T)
                    prev = (fitness, rmse)
        if stop:
            result[:16] = T.reshape(-1)
            if status != 1:
                result[16:19] = [fitness, rmse, S[1]]
                header[:] = [status, nvs, int(t_ok.sum()), int(m), k, converged, 0, 0]
            else:
                header[0] = 1
            return Result(index, result, trace, header)
        k += 1
