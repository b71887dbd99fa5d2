"""A numpy model of soft voting (include/pn2_abi.h: pn2_softmax_scores, pn2_tile_vote_scores, pn2_score_labels,
pn2_interpolate_scores), written from the header's text.  Needs neither torch nor the library.

A score row is num_class non-negative integers in units of 2^-30; rows of q are int32, accumulated scores int64."""
import numpy as np

ONE = 1 << 30
# the colour table of the label form (tf_interpolate.cpp:45-47), (r, g, b) per label 0..8; any other label: 0
COLORS = np.array([[255, 255, 255], [0, 0, 255], [128, 0, 0], [255, 0, 255], [0, 128, 0], [255, 0, 0], [128, 0, 128], [0, 0, 128],
                   [128, 128, 0]], dtype=np.uint8)


def softmax_scores(logits):
    """rule 1.  logits (rows,C) float32 -> q (rows,C) int32, the number of invalid rows"""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    q = np.zeros(x.shape, dtype=np.int32)
    invalid = 0
    for r in range(x.shape[0]):
        row = x[r].astype(np.float64)
        m = row.max() if not np.isnan(row).any() else np.nan
        if np.isnan(m) or np.isinf(m):
            invalid += 1
            continue
        with np.errstate(under="ignore"):
            e = np.exp(row - m)
        s = np.float64(0.0)
        for v in e:  # class order
            s = s + v
        q[r] = np.rint(e / s * np.float64(ONE)).astype(np.int32)  # half to even
    return q, invalid


def vote_scores(scores, sel, live, q):
    """rule 2, in place.  scores (n,C) int64; sel (b,npts), live (b,), q (b,npts,C) int32 -> the number of live rows dropped"""
    dropped = 0
    for s in range(sel.shape[0]):
        c = int(live[s])
        at, rows = sel[s, :c].astype(np.int64), q[s, :c].astype(np.int64)
        ok = (at >= 0) & (rows >= 0).all(axis=1)
        dropped += int((~ok).sum())
        np.add.at(scores, at[ok], rows[ok])
    return dropped


def score_labels(scores):
    """rule 3.  scores (n,C) int64 -> labels (n,) int32 (the first maximal class; an all-zero row: 0), confidence (n,) float32"""
    s = np.asarray(scores, dtype=np.int64)
    labels = np.argmax(s, axis=1).astype(np.int32)
    top = s[np.arange(len(s)), labels].astype(np.float64)
    total = s.sum(axis=1)
    conf = np.zeros(len(s), dtype=np.float32)
    nz = total != 0
    conf[nz] = (top[nz] / total[nz].astype(np.float64)).astype(np.float32)
    return labels, conf


def neighbours(sparse_points, dense_points, knn):
    """-> (nd, min(knn, ns)) indices of the nearest sparse points by (float64 squared L2 ((dx*dx + dy*dy) + dz*dz), index)
    ascending: brute force"""
    sp = np.asarray(sparse_points, dtype=np.float32).astype(np.float64)
    dp = np.asarray(dense_points, dtype=np.float32).astype(np.float64)
    k = min(knn, len(sp))
    out = np.zeros((len(dp), k), dtype=np.int64)
    idx = np.arange(len(sp))
    for lo in range(0, len(dp), 256):
        d = dp[lo:lo + 256, None, :] - sp[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        for i in range(len(d2)):
            out[lo + i] = np.lexsort((idx, d2[i]))[:k]
    return out


def interpolate_scores(sparse_points, sparse_scores, dense_points, knn):
    """rule 4 -> labels (nd,) int32, colours (nd,3) uint8, confidence (nd,) float32"""
    nd = len(dense_points)
    if len(sparse_points) == 0:
        return np.full(nd, -1, dtype=np.int32), np.zeros((nd, 3), dtype=np.uint8), np.zeros(nd, dtype=np.float32)
    nb = neighbours(sparse_points, dense_points, knn)
    sums = np.asarray(sparse_scores, dtype=np.int64)[nb].sum(axis=1)  # (nd, C) int64
    labels, conf = score_labels(sums)
    colors = np.zeros((nd, 3), dtype=np.uint8)
    known = labels < len(COLORS)
    colors[known] = COLORS[labels[known]]
    return labels, colors, conf
