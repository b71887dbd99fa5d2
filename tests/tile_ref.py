"""A numpy model of the tiled cover of a scene (include/pn2_abi.h: pn2_tile_plan, pn2_tile_gather, pn2_tile_vote,
pn2_tile_labels; csrc/pn2_tile.hip), written from the rule's text.  Needs neither torch nor the library."""
import numpy as np


def _min_signed(v):
    """the float64 minimum; among zeros -0.0 counts as the smaller (numpy leaves that to the order of the rows)"""
    m = np.float64(v.min())
    if m == 0.0:
        m = np.float64(-0.0) if np.signbit(v[v == 0.0]).any() else np.float64(0.0)
    return m


def plan(points, box_size_x, box_size_y, npts, phase=(0.0, 0.0), min_points=1, sample_cap=None):
    """rules 1-3.  points (n,3) float64 sorted by x -> dict(order (n,) int32, samples (n_samples or sample_cap, 4) int32,
    header (8,) int32 = [n_tiles, n_samples, skipped, status, 0, 0, 0, 0]).  With status 1 or 2 only the header's status is
    specified."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    header = np.zeros(8, dtype=np.int32)
    if not np.isfinite(p[:, :2]).all():
        header[3] = 1
        return dict(order=np.arange(n, dtype=np.int32), samples=np.zeros((0, 4), np.int32), header=header)
    ox = p[0, 0] - np.float64(phase[0])
    oy = _min_signed(p[:, 1]) - np.float64(phase[1])
    i = np.floor((p[:, 0] - ox) / np.float64(box_size_x))  # subtraction, division, floor: all float64
    j = np.floor((p[:, 1] - oy) / np.float64(box_size_y))
    if (i < 0).any() or (j < 0).any() or (i >= 2.0 ** 31).any() or (j >= 2.0 ** 31).any():
        header[3] = 2
        return dict(order=np.arange(n, dtype=np.int32), samples=np.zeros((0, 4), np.int32), header=header)
    key = (i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
    order = np.argsort(key, kind="stable").astype(np.int32)
    sk = key[order]
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    sizes = np.diff(np.concatenate([starts, [n]]))
    rows, skipped = [], 0
    for a, m in zip(starts.tolist(), sizes.tolist()):
        if m < min_points:
            skipped += m
            continue
        S = -(-m // npts)
        rows.extend([a, m, s, S] for s in range(S))
    samples = np.array(rows, dtype=np.int32).reshape(-1, 4)
    header[:3] = (len(starts), len(samples), skipped)
    if sample_cap is not None and len(samples) > sample_cap:
        header[3] = 3
        samples = samples[:sample_cap]
    return dict(order=order, samples=samples, header=header)


def sample_rows(pl, q, npts):
    """-> (sel (npts,) int32, c): the scene positions of the rows of sample q and how many of them are live"""
    a, m, s, S = (int(v) for v in pl["samples"][q])
    c = -(-(m - s) // S)
    k = np.arange(npts)
    return pl["order"][a + s + (k % c) * S].astype(np.int32), c


def batch(pl, points, colors, q0, b, npts, box_size_x, box_size_y):
    """rule 4.  -> data (b,npts,3|6) float32, sel (b,npts) int32, live (b,) int32; colors (n,3) float32 or None"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    ch = 3 if colors is None else 6
    data = np.zeros((b, npts, ch), dtype=np.float32)
    sel = np.full((b, npts), -1, dtype=np.int32)
    live = np.zeros(b, dtype=np.int32)
    ns = int(pl["header"][1]) if pl["header"][3] == 0 else 0
    if ns == 0:
        return data, sel, live
    for slot in range(b):
        q = q0 + slot
        rows, c = sample_rows(pl, min(q, ns - 1), npts)
        pts = p[rows]
        shift = np.array([_min_signed(pts[:, 0]) + np.float64(box_size_x) / 2, _min_signed(pts[:, 1]) + np.float64(box_size_y) / 2,
                          _min_signed(pts[:, 2])], dtype=np.float64)
        data[slot, :, 0:3] = (pts - shift).astype(np.float32)
        if colors is not None:
            data[slot, :, 3:6] = np.asarray(colors, dtype=np.float32)[rows]
        sel[slot] = rows
        live[slot] = c if q < ns else 0
    return data, sel, live


def vote(votes, sel, live, pred):
    """rule 5, in place.  votes (n,C) int32 -> the number of live rows dropped"""
    C = votes.shape[1]
    dropped = 0
    for q in range(sel.shape[0]):
        c = int(live[q])
        s, p = sel[q, :c].astype(np.int64), pred[q, :c].astype(np.int64)
        ok = (p >= 0) & (p < C) & (s >= 0)
        dropped += int((~ok).sum())
        np.add.at(votes, (s[ok], p[ok]), 1)
    return dropped


def labels(votes):
    """rule 6: the first maximal class; no vote at all: 0"""
    return np.argmax(votes, axis=1).astype(np.int32)


def predict_scene(points, colors, box_size_x, box_size_y, npts, num_class, predict, batch_size, phases=((0.0, 0.0),),
                  min_points=1):
    """rule 7 with predict(data (B,npts,3|6) float32) -> (B,npts) int labels.  -> labels (n,) int32, votes (n,C) int32"""
    votes = np.zeros((len(points), num_class), dtype=np.int32)
    for ph in phases:
        pl = plan(points, box_size_x, box_size_y, npts, ph, min_points)
        assert pl["header"][3] == 0
        for q0 in range(0, int(pl["header"][1]), batch_size):
            data, sel, live = batch(pl, points, colors, q0, batch_size, npts, box_size_x, box_size_y)
            vote(votes, sel, live, np.asarray(predict(data)))
    return labels(votes), votes
