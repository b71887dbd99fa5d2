"""The clouds and motions that tests/test_icp_cpu.py and tests/test_icp_gpu.py share: a three-plane corner, a known rigid motion of
it, numpy's SVD Kabsch as the independent answer, and the bound that both files hold the converged pose to."""
import numpy as np

F = np.float64


def rotation(axis, degrees):
    a = np.asarray(axis, dtype=F) / np.linalg.norm(axis)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rigid(axis, degrees, translation):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, degrees)
    T[:3, 3] = translation
    return T


def corner(seed, n=400, size=2.0):
    """n points on three mutually orthogonal square faces meeting in (3, -2, 1), and their normals"""
    rs = np.random.RandomState(seed)
    k = n // 3
    uv = rs.uniform(0, size, (n, 2))
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    pts[:k, 0], pts[:k, 1], nrm[:k, 2] = uv[:k, 0], uv[:k, 1], 1
    pts[k:2 * k, 0], pts[k:2 * k, 2], nrm[k:2 * k, 1] = uv[k:2 * k, 0], uv[k:2 * k, 1], 1
    pts[2 * k:, 1], pts[2 * k:, 2], nrm[2 * k:, 0] = uv[2 * k:, 0], uv[2 * k:, 1], 1
    return (pts + [3.0, -2.0, 1.0]).astype(np.float32), nrm.astype(np.float32)


TRUTH = rigid([1, 2, 3], 2.0, [0.06, -0.05, 0.06])  # 2 degrees and 0.1 units (0.0985)


def moved_corner(seed=0):
    """-> source, target, normals: the target is the corner, the source is the corner under inv(TRUTH), rounded to float32"""
    target, normals = corner(seed)
    inv = np.linalg.inv(TRUTH)
    source = (target.astype(F) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return source, target, normals


def kabsch(p, u):
    """numpy's answer: the rigid T with T p ~ u in the least-squares sense, by SVD"""
    pc, uc = p.mean(0), u.mean(0)
    U, _, Vt = np.linalg.svd((u - uc).T @ (p - pc))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = uc - T[:3, :3] @ pc
    return T


def corner_bound():
    """8x the deviation of numpy's SVD Kabsch on the true pairs of moved_corner() from TRUTH: the bound of the convergence
    checks here and in test_icp_gpu.py"""
    source, target, _ = moved_corner()
    return 8.0 * np.abs(kabsch(source.astype(F), target.astype(F)) - TRUTH).max()
