"""What describing the objects of a clustered cloud costs ("Object description"): one JSON line per case
and order (progress on stderr), in this one process, after a warm-up call of every shape:
  call      pn2.describe_clusters end to end (workspace and outputs allocated, seven launches): the median of --rounds
            host-clock timings, the device synchronised on both sides;
  device    pn2_cluster_describe alone on preallocated buffers: device events around --reps calls back to back, per call;
  parts     device time per call by kernel name from torch's profiler, in a pass of its own (tracing slows the host);
  torch     (a) the same quantities in torch ops on the device: float64 index_add_ moments about the cluster's box minimum,
            batched torch.linalg.eigh, scatter_reduce amin / amax for the box and the extents; timed like `call`; its centroids,
            eigenvalues and extents are compared with the library's (a tolerance: it is float64 sums in arrival order);
  host      (b) the loop a user would write: ids and points copied to the host, np.cov and np.linalg.eigh once per object; at
            most --host-objects objects are looped over (evenly spaced ids) and the loop's time is scaled up to all of them;
  peel      (c) with a TUNING build of the library loaded (PN2_HIP_LIBRARY=.../libpn2_tune.so built with -DPN2_TUNING_HOOKS):
            `device` for each (rounds, min_lanes) of --peel, alternated --alternations times in this one call; rounds = 0 is
            one atomic per lane and no wave reduction.  moments and desc of every setting are compared for equality.
The cases are those of tools/cluster_cost.py: its 120 000-point LiDAR-like frame clustered at eps = 0.5 with min_points = 10,
and its 1.5 M-point scene at eps = 0.1 -- both in the shuffled order that tool makes, and again sorted by cluster id (what a
cloud looks like after a grid sort or along a scan line: long runs of one id).
usage: python tools/describe_cost.py [--rounds 7] [--reps 20] [--cases frame scene] [--no-host] [--peel 0,1 64,2 ...]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pn2_amd as pn2  # noqa: E402
import cluster_cost  # noqa: E402

KERNELS = ("describe_clear", "describe_box", "describe_lattice", "describe_moments", "describe_axes", "describe_extent",
           "describe_finish")
HOOK_ROUNDS, HOOK_MIN_LANES = 19, 20  # pn2_debug_set of the tuning build (csrc/pn2_describe.hip)
SHIPPED = (64, 2)                     # kPeelRounds, kPeelMinLanes there


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(runs):
    return {"median": round(float(np.median(runs)), 4), "min": round(float(min(runs)), 4), "max": round(float(max(runs)), 4)}


class Raw:
    """pn2_cluster_describe on buffers allocated once"""

    def __init__(self, points, ids, count, upright):
        dev = points.device
        self.moments = torch.empty((count, 12), dtype=torch.int64, device=dev)
        self.desc = torch.empty((count, 24), dtype=torch.float64, device=dev)
        nbytes = ctypes.c_ulonglong(0)
        pn2._lib.launch("pn2_cluster_describe_workspace_size", dev, count, ctypes.byref(nbytes), stream=False)
        self.ws = torch.empty((int(nbytes.value) + 255,), dtype=torch.uint8, device=dev)
        off = (-self.ws.data_ptr()) % 256
        self.args = (dev, len(points), count, pn2._lib.ptr(points), pn2._lib.ptr(ids), int(upright), pn2._lib.ptr(self.moments),
                     pn2._lib.ptr(self.desc), self.ws.data_ptr() + off, int(nbytes.value))
        self.keep = (points, ids)

    def __call__(self):
        pn2._lib.launch("pn2_cluster_describe", *self.args)

    def device_ms(self, reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self()
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            self()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps


def parts(call, rounds):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(rounds):
            call()
        torch.cuda.synchronize()
    t = {k: 0.0 for k in KERNELS + ("other",)}
    for ev in prof.events():
        dur = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
        if dur:
            t[next((k for k in KERNELS if k in ev.name), "other")] += dur
    return {k: round(v / rounds / 1e3, 4) for k, v in t.items()}


def torch_ops(points, ids, count, marks=None):
    """(a) -> size, centroid, eigenvalues (descending), axes (rows), lo, hi: torch ops only, float64.  marks: a list that gets the
    host clock, the device synchronised, at the start, behind the moments, behind eigh and at the end"""
    def mark():
        if marks is not None:
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
    mark()
    p = points.to(torch.float64)
    member = (ids >= 0) & (ids < count) & torch.isfinite(points).all(1)
    c = torch.where(member, ids, torch.zeros_like(ids)).long()
    w = member.to(torch.float64)[:, None]
    idx3 = c[:, None].expand(-1, 3)
    origin = torch.full((count, 3), float("inf"), dtype=torch.float64, device=p.device).scatter_reduce(
        0, idx3, torch.where(member[:, None], p, torch.full_like(p, float("inf"))), "amin")
    d = torch.where(member[:, None], p - origin[c], torch.zeros_like(p))
    size = torch.zeros((count,), dtype=torch.float64, device=p.device).index_add_(0, c, w[:, 0])
    s1 = torch.zeros((count, 3), dtype=torch.float64, device=p.device).index_add_(0, c, d)
    s2 = torch.zeros((count, 9), dtype=torch.float64, device=p.device).index_add_(0, c, (d[:, :, None] * d[:, None, :]).reshape(-1, 9))
    mean = s1 / size[:, None]
    cov = s2.reshape(count, 3, 3) / size[:, None, None] - mean[:, :, None] * mean[:, None, :]
    mark()
    lam, vec = torch.linalg.eigh(cov)
    mark()
    lam, axes = lam.flip(1), vec.flip(2).transpose(1, 2)  # descending; rows
    centroid = origin + mean
    t = torch.einsum("nka,na->nk", axes[c], p - centroid[c])
    inf = torch.full_like(t, float("inf"))
    lo = torch.full((count, 3), float("inf"), dtype=torch.float64, device=p.device).scatter_reduce(
        0, idx3, torch.where(member[:, None], t, inf), "amin")
    hi = torch.full((count, 3), float("-inf"), dtype=torch.float64, device=p.device).scatter_reduce(
        0, idx3, torch.where(member[:, None], t, -inf), "amax")
    mark()
    return size, centroid, lam, axes, lo, hi


def say(*what):
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


T0 = time.perf_counter()


def host_loop(points, ids, count, most):
    """(b) -> seconds, objects looped over: the copy to the host, the grouping and one np.cov / np.linalg.eigh per object, the
    loop's share scaled from `most` objects to all when there are more"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, i = points.cpu().numpy().astype(np.float64), ids.cpu().numpy()
    order = np.argsort(i, kind="stable")
    bounds = np.searchsorted(i[order], np.arange(count + 1))
    some = np.unique(np.linspace(0, count - 1, min(count, most)).astype(np.int64))
    t1 = time.perf_counter()
    out = []
    for c in some:
        q = p[order[bounds[c]:bounds[c + 1]]]
        centroid = q.mean(0)
        lam, vec = np.linalg.eigh(np.cov(q.T, bias=True)) if len(q) > 1 else (np.zeros(3), np.eye(3))
        t = (q - centroid) @ vec
        out.append((centroid, lam, t.min(0), t.max(0)))
    t2 = time.perf_counter()
    return (t1 - t0) + (t2 - t1) * count / len(some), len(some)


def peel_ab(raw, settings, alternations, reps):
    dbg = pn2._lib._raw.pn2_debug_set
    runs = {s: [] for s in settings}
    want = None
    for _ in range(alternations):
        for rounds, min_lanes in settings:
            assert dbg(HOOK_ROUNDS, rounds) == 0 and dbg(HOOK_MIN_LANES, min_lanes) == 0
            runs[(rounds, min_lanes)].append(raw.device_ms(reps))
            got = (raw.moments.cpu().numpy().tobytes(), raw.desc.cpu().numpy().tobytes())
            want = want or got
            assert got == want, "a peel setting changed the result"
    out = {}
    for (rounds, min_lanes), r in runs.items():
        assert dbg(HOOK_ROUNDS, rounds) == 0 and dbg(HOOK_MIN_LANES, min_lanes) == 0
        out["%d,%d" % (rounds, min_lanes)] = dict(stats(r), moments_kernel_ms=parts(raw, 5)["describe_moments"])
    assert dbg(HOOK_ROUNDS, SHIPPED[0]) == 0 and dbg(HOOK_MIN_LANES, SHIPPED[1]) == 0  # as the library ships, for what follows
    return out


def torch_baseline(out, boxes, d_pts, ids, count, args):
    # (a)
    size, centroid, lam, _, lo, hi = torch_ops(d_pts, ids, count)
    say("torch ops warm")
    out["torch_ms"] = stats([wall_ms(lambda: torch_ops(d_pts, ids, count)) for _ in range(args.torch_rounds)])
    say("torch ops timed")
    out["torch_over_call"] = round(out["torch_ms"]["median"] / out["call_ms"]["median"], 1)
    marks = []
    torch_ops(d_pts, ids, count, marks)
    out["torch_parts_ms"] = dict(zip(("moments", "eigh", "extents"), (round(v * 1e3, 3) for v in np.diff(marks))))
    full = boxes.size > 3
    scale = (boxes.hi - boxes.lo).amax(1, keepdim=True).clamp_min(1e-30)
    out["torch_agrees"] = {
        "size": bool(torch.equal(size.long(), boxes.size)),
        "centroid_rel": float(((centroid - boxes.centroid).abs() / scale)[full].max()),
        # (a) takes the full eigenproblem; upright keeps z apart: compare the trace, which both preserve
        "variance_trace_rel": float((((lam.sum(1) - boxes.variance.sum(1)).abs()) / (scale[:, 0] ** 2))[full].max())}


def case(name, order, args, dev):
    make, kw = cluster_cost.CASES[name]
    points, labels = make()
    d_pts, d_lab = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)
    clusters = pn2.euclidean_clusters(d_pts, labels=d_lab, **kw)
    ids, count = clusters.ids, clusters.count
    if order == "sorted":
        at = torch.argsort(ids, stable=True)
        d_pts, ids = d_pts[at].contiguous(), ids[at].contiguous()
    out = {"case": name, "order": order, "points": len(points), "clusters": count, "largest": int(clusters.size.max()),
           "points_in_clusters": int((ids >= 0).sum())}

    def call():
        return pn2.describe_clusters(d_pts, (ids, count), upright=True)

    say(name, order, "clustered:", count, "objects")
    boxes = call()  # the warm-up of every shape timed below
    out["call_ms"] = stats([wall_ms(call) for _ in range(args.rounds)])
    raw = Raw(d_pts, ids, count, True)
    out["device_ms"] = stats([raw.device_ms(args.reps) for _ in range(args.rounds)])
    try:
        out["parts_ms"] = parts(raw, args.rounds)
    except Exception as err:  # no tracer in this build of torch
        out["parts_ms"], out["parts_error"] = None, repr(err)[:200]
    say("library timed")
    if not args.no_torch:
        torch_baseline(out, boxes, d_pts, ids, count, args)
    if not args.no_host:
        seconds, looped = host_loop(d_pts, ids, count, args.host_objects)
        out["host_s"], out["host_objects_looped"] = round(seconds, 3), looped
        out["host_over_call"] = round(seconds * 1e3 / out["call_ms"]["median"], 1)
        say("host loop")
    if hasattr(pn2._lib._raw, "pn2_debug_set"):
        out["peel"] = peel_ab(raw, [tuple(int(v) for v in s.split(",")) for s in args.peel], args.alternations, args.reps)
        say("peel settings")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(cluster_cost.CASES), choices=list(cluster_cost.CASES))
    ap.add_argument("--orders", nargs="+", default=["shuffled", "sorted"], choices=["shuffled", "sorted"])
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--host-objects", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--peel", nargs="+", default=["0,1", "64,2"], help="rounds,min_lanes settings for the tuning build's A/B")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.cases:
        for order in args.orders:
            out = case(name, order, args, dev)
            out["device"], out["library"] = torch.cuda.get_device_name(dev), os.path.basename(pn2._lib.LIB_PATH)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
