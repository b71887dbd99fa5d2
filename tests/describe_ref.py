"""The numpy / Python-int model of pn2_cluster_describe and pn2_box_wireframe, written from the rules in include/pn2_abi.h
("Object description").  Every float64 operation below is one IEEE operation in the association the header writes (numpy does
not contract a multiply and an add), the moments are Python ints, and minima / maxima of doubles go through the same
order-preserving 64-bit key the library uses, so the model and the library are compared for equality, bit for bit.

    moments, desc = describe(points, ids, nclusters, upright)      # (C,12) int64, (C,24) float64
    points, owner = wireframe(desc, per_edge)                      # (C*12*per_edge,3) float32, (C*12*per_edge,) int32
"""
import numpy as np

F = np.float64
SWEEPS = 8
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))  # (p, r, k)


def lattice_bits(m):
    """Q = min(20, (62 - bitlen(m)) >> 1)"""
    return min(20, (62 - int(m).bit_length()) >> 1)


def ordered_key(v):
    """float64 array -> uint64 keys with the same order, -0.0 directly below +0.0 (csrc/pn2_ordered.h, ordered_key)"""
    k = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(k >> np.uint64(63), ~k, k | np.uint64(1 << 63))


def ordered_to_double(k):
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def key_min(v):
    return ordered_to_double(np.array([ordered_key(v).min()]))[0]


def key_max(v):
    return ordered_to_double(np.array([ordered_key(v).max()]))[0]


def rotate(A, V, p, r, k):
    """one Jacobi rotation on the pair (p, r) of the symmetric A (only A[min,max] entries are kept), in place"""
    def at(i, j):
        return (i, j) if i < j else (j, i)
    apr = A[at(p, r)]
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
    A[at(p, r)] = F(0.0)
    akp, akr = A[at(k, p)], A[at(k, r)]
    A[at(k, p)] = c * akp - s * akr
    A[at(k, r)] = s * akp + c * akr
    for i in range(3):
        vp, vr = V[i, p], V[i, r]
        V[i, p] = c * vp - s * vr
        V[i, r] = s * vp + c * vr


def fix_sign(v):
    at = 0
    for j in (1, 2):
        if np.abs(v[j]) > np.abs(v[at]):
            at = j
    return -v if v[at] < 0.0 else v


def sorted_pairs(diag, cols):
    """descending by diagonal entry, equal values keep the lower column first: a bubble sort that swaps on a strict 'less'"""
    diag, cols = list(diag), list(cols)
    n = len(diag)
    for done in range(n - 1):
        for j in range(n - 1 - done):
            if diag[j] < diag[j + 1]:
                diag[j], diag[j + 1] = diag[j + 1], diag[j]
                cols[j], cols[j + 1] = cols[j + 1], cols[j]
    return diag, cols


def axes_of(A, upright):
    """A (3,3) float64, upper triangle used -> lambda (3,), a0, a1, a2, and A after the rotations (for the tests)"""
    A = np.array(A, dtype=F)
    V = np.eye(3, dtype=F)
    if upright:
        azz = A[2, 2]
        rotate(A, V, 0, 1, 2)
        lam, cols = sorted_pairs([A[0, 0], A[1, 1]], [V[:, 0].copy(), V[:, 1].copy()])
        a0 = fix_sign(cols[0])
        a1 = np.array([-a0[1], a0[0], F(0.0)], dtype=F)
        a2 = np.array([0.0, 0.0, 1.0], dtype=F)
        return np.array(lam + [azz], dtype=F), a0, a1, a2, A
    for _ in range(SWEEPS):
        for p, r, k in PAIRS:
            rotate(A, V, p, r, k)
    lam, cols = sorted_pairs([A[0, 0], A[1, 1], A[2, 2]], [V[:, j].copy() for j in range(3)])
    a0, a1 = fix_sign(cols[0]), fix_sign(cols[1])
    a2 = np.array([a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]], dtype=F)
    return np.array(lam, dtype=F), a0, a1, a2, A


def lattice(p64, m):
    """the members as float64 (m,3) -> o (3,), Q, x, h"""
    o = np.array([key_min(p64[:, a]) for a in range(3)], dtype=F)  # -0.0 below +0.0, as the library's ordered minimum
    E = (np.array([key_max(p64[:, a]) for a in range(3)], dtype=F) - o).max()
    Q = lattice_bits(m)
    x = int(np.frexp(E)[1]) if E > 0 else Q
    return o, Q, x, np.ldexp(F(1.0), x - Q)


def moments_of(q):
    """q (m,3) Python-int-exact lattice coordinates (int64) -> S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz as Python ints"""
    cols = [[int(v) for v in q[:, a]] for a in range(3)]
    out = [sum(c) for c in cols]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append(sum(u * v for u, v in zip(cols[a], cols[b])))
    return out


def covariance(S, m):
    """the moments (Python ints) -> the means in lattice units (3,), A (3,3) float64 (upper triangle)"""
    md = F(m)
    mean = [F(S[a]) / md for a in range(3)]
    A = np.zeros((3, 3), dtype=F)
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[a, b] = F(S[3 + j]) / md - mean[a] * mean[b]
    return mean, A


def describe(points, ids, nclusters, upright):
    points = np.asarray(points, dtype=np.float32)
    ids = np.asarray(ids)
    moments = np.zeros((nclusters, 12), dtype=np.int64)
    desc = np.full((nclusters, 24), np.nan, dtype=F)
    finite = np.isfinite(points).all(axis=1)
    for c in range(nclusters):
        p64 = points[(ids == c) & finite].astype(F)
        m = len(p64)
        if m == 0:
            continue
        o, Q, x, h = lattice(p64, m)
        q = np.rint((p64 - o) / h).astype(np.int64)
        S = moments_of(q)
        assert all(abs(v) < 2 ** 62 for v in S)
        moments[c] = [m] + S + [Q, x]
        mean, A = covariance(S, m)
        centroid = np.array([o[a] + mean[a] * h for a in range(3)], dtype=F)
        lam, a0, a1, a2, _ = axes_of(A, upright)
        d = p64 - centroid
        lo, hi = np.empty(3, dtype=F), np.empty(3, dtype=F)
        for k, a in enumerate((a0, a1, a2)):
            t = (a[0] * d[:, 0] + a[1] * d[:, 1]) + a[2] * d[:, 2]
            lo[k], hi[k] = key_min(t), key_max(t)
        g = F(0.5) * (lo + hi)
        center = np.array([centroid[a] + ((a0[a] * g[0] + a1[a] * g[1]) + a2[a] * g[2]) for a in range(3)], dtype=F)
        desc[c] = np.concatenate([centroid, lam * (h * h), a0, a1, a2, lo, hi, center])
    return moments, desc


def edge_corners():
    """the 12 (A, B) corner pairs in the header's order"""
    out = []
    for k in range(3):
        u, w = [b for b in range(3) if b != k]
        for v in range(4):
            a = ((v & 1) << u) | ((v >> 1) << w)
            out.append((a, a | (1 << k)))
    return out


def corner(row, j):
    e = [row[18 + k] if (j >> k) & 1 else row[15 + k] for k in range(3)]
    return np.array([row[a] + ((row[6 + a] * e[0] + row[9 + a] * e[1]) + row[12 + a] * e[2]) for a in range(3)], dtype=F)


def wireframe(desc, per_edge):
    desc = np.asarray(desc, dtype=F)
    C = len(desc)
    f = np.arange(per_edge, dtype=F) / F(per_edge - 1)
    points = np.empty((C, 12, per_edge, 3), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for c in range(C):
            for e, (a, b) in enumerate(edge_corners()):
                A, B = corner(desc[c], a), corner(desc[c], b)
                points[c, e] = (A[None, :] + (B - A)[None, :] * f[:, None]).astype(np.float32)
    return points.reshape(-1, 3), np.repeat(np.arange(C, dtype=np.int32), 12 * per_edge)
