"""What grouping labelled points into objects costs ("Euclidean clustering"): one JSON line with, per
case, in this one process, after a warm-up call of the same shape:
  call      pn2.euclidean_clusters end to end (workspace allocation, pn2_cluster_points, the header read, pn2_cluster_stats):
            the median of --rounds host-clock timings, the device synchronised on both sides;
  parts     device time per call by kernel name from torch's profiler, in a pass of its own (tracing slows the host): grid
            (init, minimum, keys, the radix sort, the gather), union, flatten + number (flatten, flag, offsets, number, ids), stats;
  host      scipy.spatial.cKDTree.query_pairs + scipy.sparse.csgraph.connected_components on the same float32 points, per label,
            one timing; its ids, numbered as the device numbers them, are compared with the device's.  Without scipy the tool
            says that there is no baseline.
The cases: a synthetic 120 000-point LiDAR-like frame (rings on a ground plane and boxes on it, nine labels) at eps = 0.5 with
min_points = 10, and a 1.5 M-point synthetic scene (a 60 m x 60 m ground sheet with 400 objects on it) at eps = 0.1.
usage: python tools/cluster_cost.py [--rounds 7] [--cases frame scene] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

GRID = ("cluster_init", "grid_min", "grid_key", "grid_gather")  # the last three: pn2_cell_grid.h
NUMBER = ("cluster_flatten", "cluster_flag", "cluster_offsets", "cluster_number", "cluster_ids")


def frame(n=120000, seed=0):
    """a LiDAR-like frame: 64 rings on the ground around the origin (label 1), 60 boxes of 2 x 4.5 x 1.6 m (label 8) and 40 posts
    (label 5) standing on it"""
    rs = np.random.RandomState(seed)
    n_obj = n // 3
    ring = rs.randint(0, 64, n - n_obj)
    r = 3.0 * 1.055 ** ring
    a = rs.uniform(0, 2 * np.pi, n - n_obj)
    ground = np.stack([r * np.cos(a), r * np.sin(a), rs.normal(0, 0.02, n - n_obj)], 1)
    which = rs.randint(0, 100, n_obj)
    centre = rs.uniform(-40, 40, (100, 2))
    size = np.where(np.arange(100)[:, None] < 60, [[2.0, 4.5, 1.6]], [[0.3, 0.3, 3.0]])
    obj = np.concatenate([centre[which], np.zeros((n_obj, 1))], 1) + rs.uniform(0, 1, (n_obj, 3)) * size[which] + [0, 0, 0.3]
    points = np.concatenate([ground, obj]).astype(np.float32)
    labels = np.concatenate([np.ones(n - n_obj), np.where(which < 60, 8, 5)]).astype(np.int32)
    order = rs.permutation(n)
    return points[order], labels[order]


def scene(n=1500000, seed=1):
    """a static scene: a 60 m x 60 m ground sheet (label 1) and 400 objects of 1.5 m (labels 2 .. 8) on it"""
    rs = np.random.RandomState(seed)
    n_obj = n // 2
    ground = np.concatenate([rs.uniform(0, 60, (n - n_obj, 2)), rs.normal(0, 0.01, (n - n_obj, 1))], 1)
    which = rs.randint(0, 400, n_obj)
    centre = rs.uniform(0, 60, (400, 2))
    obj = np.concatenate([centre[which], np.full((n_obj, 1), 0.5)], 1) + rs.uniform(0, 1.5, (n_obj, 3))
    points = np.concatenate([ground, obj]).astype(np.float32)
    labels = np.concatenate([np.ones(n - n_obj), 2 + which % 7]).astype(np.int32)
    order = rs.permutation(n)
    return points[order], labels[order]


CASES = {"frame": (frame, dict(eps=0.5, min_points=10)), "scene": (scene, dict(eps=0.1, min_points=1))}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def parts(call, rounds):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(rounds):
            call()
        torch.cuda.synchronize()
    t = {"grid": 0.0, "union": 0.0, "flatten_number": 0.0, "stats": 0.0, "other": 0.0}
    for ev in prof.events():
        dur = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
        if not dur:
            continue
        name = ev.name
        which = ("grid" if any(k in name for k in GRID) or "adix" in name or "onesweep" in name.lower() else
                 "union" if "cluster_union" in name else "flatten_number" if any(k in name for k in NUMBER) else
                 "stats" if "stats_" in name else "other")
        t[which] += dur
    return {k: round(v / rounds / 1e3, 4) for k, v in t.items()}


def host_baseline(points, labels, eps, min_points):
    """-> seconds, ids in the device's numbering (kept components by ascending first index)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    n = len(points)
    rows, cols = [], []
    for c in np.unique(labels[labels >= 0]):
        at = np.nonzero(labels == c)[0]
        pairs = cKDTree(points[at].astype(np.float64)).query_pairs(float(np.float32(eps)), output_type="ndarray")
        rows.append(at[pairs[:, 0]])
        cols.append(at[pairs[:, 1]])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, comp = connected_components(coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n)), directed=False)
    seconds = time.perf_counter() - t0
    size = np.bincount(comp)
    first = np.full(len(size), n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    kept = (size >= min_points) & (labels[first] >= 0)
    rank = np.full(len(size), -1, dtype=np.int64)
    rank[np.argsort(np.where(kept, first, n), kind="stable")[:kept.sum()]] = np.arange(kept.sum())
    return seconds, np.where(labels >= 0, rank[comp], -1)


def case(name, rounds, dev, host):
    make, kw = CASES[name]
    points, labels = make()
    d_pts, d_lab = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)

    def call():
        return pn2.euclidean_clusters(d_pts, labels=d_lab, **kw)

    c = call()  # the warm-up of every shape timed below
    out = {"case": name, "points": len(points), "clusters": c.count, "largest": int(c.size.max()) if c.count else 0,
           "points_in_clusters": int((c.ids >= 0).sum())}
    out.update(kw)
    runs = [wall_ms(call) for _ in range(rounds)]
    out["call_ms"] = {"median": round(float(np.median(runs)), 3), "runs": [round(r, 3) for r in runs]}
    try:
        out["parts_ms"] = parts(call, rounds)
    except Exception as err:  # no tracer in this build of torch: the whole call above stands alone
        out["parts_ms"], out["parts_error"] = None, repr(err)[:200]
    if host:
        try:
            seconds, ids = host_baseline(points, labels, kw["eps"], kw["min_points"])
            # the KD-tree measures sqrt(sum) <= eps in its own arithmetic: a pair exactly on the threshold may differ
            out["host_s"], out["host_same_ids"] = round(seconds, 3), bool(np.array_equal(ids, c.ids.cpu().numpy()))
            out["host_over_call"] = round(seconds * 1e3 / out["call_ms"]["median"], 1)
        except ImportError:
            out["host_s"] = "no baseline: scipy does not import"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"cases": [case(name, args.rounds, dev, not args.no_host) for name in args.cases]}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
