"""The numpy model of Euclidean clustering (include/pn2_abi.h: pn2_cluster_points, pn2_cluster_stats, pn2_cluster_colors).
numpy only.  All pairs in float64, an edge list, then minimum-label propagation with pointer jumping until nothing changes: no
grid and no union-find, so it shares nothing with the kernels but the rules.  Meant for n <= 4097 (the pair matrix is n^2)."""
import numpy as np

GREY = (96, 96, 96)


def valid_mask(points, labels=None):
    points = np.asarray(points, dtype=np.float32)
    ok = np.isfinite(points).all(axis=1)
    if labels is not None:
        ok &= np.asarray(labels) >= 0
    return ok


def edges(points, eps, labels=None, block=512):
    """-> (m,2) int64 pairs i < j of linked points"""
    points = np.asarray(points, dtype=np.float32)
    n = len(points)
    ok = valid_mask(points, labels)
    p = points.astype(np.float64)
    eps2 = np.float64(np.float32(eps)) * np.float64(np.float32(eps))
    lab = None if labels is None else np.asarray(labels, dtype=np.int64)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, block):
            b = min(n, a + block)
            dx = p[a:b, None, 0] - p[None, :, 0]
            dy = p[a:b, None, 1] - p[None, :, 1]
            dz = p[a:b, None, 2] - p[None, :, 2]
            link = ((dx * dx + dy * dy) + dz * dz) <= eps2
            link &= ok[a:b, None] & ok[None, :]
            if lab is not None:
                link &= lab[a:b, None] == lab[None, :]
            i, j = np.nonzero(link)
            i = i + a
            keep = i < j
            out.append(np.stack([i[keep], j[keep]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def components(n, pairs):
    """-> (n,) the lowest index of every point's component, and the number of rounds it took"""
    low = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        new = low.copy()
        if len(pairs):
            m = np.minimum(low[pairs[:, 0]], low[pairs[:, 1]])
            np.minimum.at(new, pairs[:, 0], m)
            np.minimum.at(new, pairs[:, 1], m)
            np.minimum.at(new, low[pairs[:, 0]], m)  # hook the representatives too
            np.minimum.at(new, low[pairs[:, 1]], m)
        while True:  # pointer jumping
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, low):
            return low, rounds
        low = new


def cluster(points, eps, labels=None, min_points=1, max_points=0):
    """-> ids (n,) int32, header (8,) int32"""
    points = np.asarray(points, dtype=np.float32)
    n = len(points)
    ok = valid_mask(points, labels)
    low, _ = components(n, edges(points, eps, labels))
    size = np.bincount(low[ok], minlength=n)
    is_root = ok & (low == np.arange(n))
    kept = is_root & (size >= min_points) & ((size <= max_points) if max_points else True)
    number = np.where(kept, np.cumsum(kept) - 1, -1)
    ids = np.where(ok, number[low], -1).astype(np.int32)
    header = np.array([0, kept.sum(), is_root.sum(), ok.sum(), size[kept].sum(), 0, 0, 0], dtype=np.int32)
    return ids, header


def _ordered(a):
    """the order-preserving uint32 image of float32 values: -0.0 below +0.0"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def stats(points, ids, labels=None, count=None):
    """-> first, size, label (count,) int32, bbox (count,6) float32"""
    points = np.asarray(points, dtype=np.float32)
    ids = np.asarray(ids)
    count = int(ids.max()) + 1 if count is None else count
    first = np.full(count, 2 ** 31 - 1, dtype=np.int32)
    size = np.zeros(count, dtype=np.int32)
    label = np.zeros(count, dtype=np.int32)
    bbox = np.zeros((count, 6), dtype=np.float32)
    for c in range(count):
        at = np.nonzero(ids == c)[0]
        first[c], size[c] = at[0], len(at)
        if labels is not None:
            label[c] = labels[at[0]]
        for a in range(3):
            col = points[at, a]
            key = _ordered(col)
            bbox[c, a], bbox[c, 3 + a] = col[np.argmin(key)], col[np.argmax(key)]
    return first, size, label, bbox


def colors(ids):
    """-> (n,3) uint8"""
    ids = np.asarray(ids, dtype=np.int64)
    with np.errstate(over="ignore"):
        h = (ids & 0xFFFFFFFF).astype(np.uint32) * np.uint32(0x9E3779B1)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x85EBCA77)
        h ^= h >> np.uint32(13)
    hue = (h % np.uint32(1536)).astype(np.int64)
    s, f = hue >> 8, hue & 255
    z, full = np.zeros_like(f), np.full_like(f, 255)
    table = [(full, f, z), (255 - f, full, z), (z, full, f), (z, 255 - f, full), (f, z, full), (full, z, 255 - f)]
    out = np.zeros((len(ids), 3), dtype=np.uint8)
    for k in range(3):
        out[:, k] = np.choose(s, [t[k] for t in table]).astype(np.uint8)
    out[ids < 0] = GREY
    return out
