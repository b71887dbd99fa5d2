"""What finding the dominant plane of a cloud costs ("Plane segmentation"): one JSON line with, per case, in
this one process, after a warm-up call of the same shape:
  call      pn2.segment_plane end to end (workspace allocation, pn2_plane_ransac, the header read, the normalised model): the
            median of --rounds host-clock timings, the device synchronised on both sides;
  score     pn2.score_planes alone over as many planes as the case has trials (the hot path on its own), timed the same way;
  parts     device time per call of `call` by kernel name from torch's profiler, in a pass of its own (tracing slows the host):
            compact (flag, offsets, compact), hypo, score (clear, score), select (select, finish), mask;
  host      the numpy model of the rules, vectorised over points, one plane at a time (tests/plane_ref.py's order of operations,
            repeated here so that the tool stands alone), run once; its header is compared with the device's.
The cases: the 120 000-point LiDAR-like frame of tools/cluster_cost.py at 1024 trials (thr 0.1, axis z within 15 degrees), and its
1.5 M-point synthetic scene at 4096 trials (thr 0.03).  For the frame it also gives the clustering of tools/cluster_cost.py's
case (eps 0.5, min_points 10, every label) with and without the ground's inliers: call time, clusters, the largest object.
--host-trials K scores only the first K non-void trials on the host and scales its time up to all of them (the 1.5 M-point case
takes minutes otherwise); the result is then not compared.
usage: python tools/plane_cost.py [--rounds 7] [--cases frame scene] [--no-host] [--host-trials K]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pn2_amd as pn2  # noqa: E402
from cluster_cost import frame, scene, wall_ms  # noqa: E402

PARTS = {"compact": ("plane_flag", "plane_offsets", "plane_compact"), "hypo": ("plane_hypo",),
         "score": ("plane_clear", "plane_score"), "select": ("plane_select", "plane_finish"), "mask": ("plane_mask",)}
CASES = {"frame": (frame, dict(distance_threshold=0.1, trials=1024, seed=0, axis=(0.0, 0.0, 1.0), max_angle=15.0)),
         "scene": (scene, dict(distance_threshold=0.03, trials=4096, seed=0))}
CLUSTER = dict(eps=0.5, min_points=10)


def parts(call, rounds):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(rounds):
            call()
        torch.cuda.synchronize()
    t = dict.fromkeys(list(PARTS) + ["other"], 0.0)
    for ev in prof.events():
        dur = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
        if not dur:
            continue
        which = [k for k, names in PARTS.items() if any(nm in ev.name for nm in names)]
        t[which[0] if which else "other"] += dur
    return {k: round(v / rounds / 1e3, 4) for k, v in t.items()}


def timed(call, rounds):
    runs = [wall_ms(call) for _ in range(rounds)]
    return {"median": round(float(np.median(runs)), 3), "min": round(min(runs), 3), "max": round(max(runs), 3),
            "runs": [round(r, 3) for r in runs]}


def host_model(points, thr, trials, seed, axis=None, max_angle=None, scored=None):
    """the rules of include/pn2_abi.h in numpy, a plane at a time over all points; only the first `scored` trials are scored
    when it is given -> seconds, [count, trial, non-void trials]"""
    U = np.uint64

    def fmix(x):
        x = x ^ (x >> U(33))
        x = x * U(0xFF51AFD7ED558CCD)
        x = x ^ (x >> U(33))
        x = x * U(0xC4CEB9FE1A85EC53)
        return x ^ (x >> U(33))

    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        valid = np.nonzero(np.isfinite(points).all(axis=1))[0]
        h = fmix(np.array([seed], dtype=U) + U(0x9E3779B97F4A7C15))
        h = fmix(h ^ U(0x2545F4914F6CDD1D))
        h = fmix(h ^ U(0x632BE59BD9B4E019))
        ranks = fmix(h ^ fmix(np.arange(3 * trials, dtype=U) + U(2 ** 45) + U(0x8CB92BA72F3D8DD7))) % U(len(valid))
        sample = valid[ranks.astype(np.int64).reshape(trials, 3)]
        P = points[valid].astype(np.float64)
        A, B, C = (points[sample[:, j]].astype(np.float64) for j in range(3))
        u, v = B - A, C - A
        nrm = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                        u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        live = np.isfinite(nn) & (nn > 0)
        if axis is not None:
            ax = np.array(axis, dtype=np.float64)
            dt = (nrm[:, 0] * ax[0] + nrm[:, 1] * ax[1]) + nrm[:, 2] * ax[2]
            live &= dt * dt >= (math.cos(math.radians(max_angle)) ** 2 * nn) * ((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
        thr2 = np.float64(np.float32(thr)) * np.float64(np.float32(thr))
        counts = np.zeros(trials, dtype=np.int64)
        for t in np.nonzero(live)[0][:scored]:
            e = (nrm[t, 0] * (P[:, 0] - A[t, 0]) + nrm[t, 1] * (P[:, 1] - A[t, 1])) + nrm[t, 2] * (P[:, 2] - A[t, 2])
            counts[t] = np.count_nonzero(e * e <= thr2 * nn[t])
    best = int(np.argmax(counts))
    return time.perf_counter() - t0, [int(counts[best]), best, int(live.sum())]


def clustering(d_pts, d_lab, exclude, rounds):
    labels = d_lab if exclude is None else torch.where(exclude, torch.full_like(d_lab, -1), d_lab)

    def call():
        return pn2.euclidean_clusters(d_pts, labels=labels, **CLUSTER)

    c = call()
    return {"clusters": c.count, "largest": int(c.size.max()) if c.count else 0, "points_in_clusters": int((c.ids >= 0).sum()),
            "call_ms": timed(call, rounds)}


def case(name, rounds, dev, host, host_trials):
    make, kw = CASES[name]
    points, labels = make()
    d_pts, d_lab = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)

    def call():
        return pn2.segment_plane(d_pts, **kw)

    plane = call()  # the warm-up of every shape timed below
    out = {"case": name, "points": len(points), "status": plane.status, "inliers": plane.count, "trial": plane.trial,
           "model": [round(v, 6) for v in plane.model.tolist()]}
    out.update({k: v for k, v in kw.items()})
    out["call_ms"] = timed(call, rounds)
    rs = np.random.RandomState(3)
    at = rs.randint(0, len(points), (kw["trials"], 3))
    P = points.astype(np.float64)
    planes = torch.from_numpy(np.concatenate([P[at[:, 0]], np.cross(P[at[:, 1]] - P[at[:, 0]], P[at[:, 2]] - P[at[:, 0]])], 1)).to(dev)

    def score():
        return pn2.score_planes(d_pts, planes, kw["distance_threshold"])

    score()
    out["score_ms"] = timed(score, rounds)
    out["score_pairs_per_s"] = round(len(points) * kw["trials"] / (out["score_ms"]["median"] * 1e-3), -6)
    try:
        out["parts_ms"] = parts(call, rounds)
    except Exception as err:  # no tracer in this build of torch: the whole call above stands alone
        out["parts_ms"], out["parts_error"] = None, repr(err)[:200]
    if host:
        seconds, found = host_model(points, kw["distance_threshold"], kw["trials"], kw["seed"], kw.get("axis"), kw.get("max_angle"),
                                    host_trials)
        if host_trials is None or host_trials >= found[2]:
            out["host_s"], out["host_same_result"] = round(seconds, 3), found[:2] == [plane.count, plane.trial]
        else:  # a share of the non-void trials was scored: the time is scaled up to all of them, and says so
            seconds *= found[2] / host_trials
            out["host_s"], out["host_scored_trials"] = round(seconds, 3), host_trials
        out["host_over_call"] = round(seconds * 1e3 / out["call_ms"]["median"], 1)
    if name == "frame":
        out["clustering"] = {"with_ground": clustering(d_pts, d_lab, None, rounds),
                             "ground_removed": clustering(d_pts, d_lab, plane.inliers, rounds)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-trials", type=int, default=None, help="score only this many trials on the host and scale its time up")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"cases": [case(name, args.rounds, dev, not args.no_host, args.host_trials) for name in args.cases]}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
