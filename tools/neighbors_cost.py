"""What fixed-radius neighbourhoods cost ("Fixed-radius neighbourhoods"): one JSON line per case (progress on
stderr), in this one process, after a warm-up call of every shape:
  call      pn2.radius_neighborhoods end to end (outputs and workspace allocated, the launches, the header read): --rounds
            host-clock timings, the device synchronised on both sides: median, smallest, largest;
  device    pn2_radius_neighborhoods alone on preallocated buffers: device events around --reps calls back to back, per call;
  parts     device time per call by kernel name from torch's profiler, in a pass of its own (tracing slows the host): grid (init,
            minimum, keys, the radix sort, the gather), scan, header;
  host      scipy.spatial.cKDTree.query_ball_point over every point, then np.cov / np.linalg.eigh per point, one timing; the
            per-point loop runs over at most --host-points points (evenly spaced) and its time is scaled up to all of them.  Its
            counts are compared with the device's.  Without scipy the tool says that there is no baseline;
  variants  with a TUNING build of the library loaded (PN2_HIP_LIBRARY=.../libpn2_tune.so built with -DPN2_TUNING_HOOKS):
            `device` for the lane path alone (hook 21 = 1) and for auto (hook 21 = 0) with kSpan (hook 22) of --spans, alternated
            --alternations times in this one call; every output of every setting is compared for equality.
The cases are those of tools/cluster_cost.py: its 120 000-point LiDAR-like frame at radius 0.5 and its 1.5 M-point scene at
radius 0.1.  No time is asserted anywhere.
usage: python tools/neighbors_cost.py [--rounds 7] [--reps 10] [--cases frame scene] [--no-host] [--spans 0 1 2 4 8]"""
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

RADIUS = {"frame": 0.5, "scene": 0.1}
GRID = ("radius_init", "grid_min", "grid_key", "grid_gather")  # the last three: pn2_cell_grid.h
HOOK_VARIANT, HOOK_SPAN = 21, 22  # pn2_debug_set of the tuning build (csrc/pn2_neighbors.hip)
SHIPPED_SPAN = 8                  # kSpan there
T0 = time.perf_counter()


def say(*what):
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(runs):
    return {"median": round(float(np.median(runs)), 4), "min": round(float(min(runs)), 4), "max": round(float(max(runs)), 4)}


class Raw:
    """pn2_radius_neighborhoods on buffers allocated once: every output asked for, the viewpoint at the origin"""

    def __init__(self, points, radius):
        dev, n = points.device, len(points)
        self.count = torch.empty((n,), dtype=torch.int32, device=dev)
        self.moments = torch.empty((n, 9), dtype=torch.int64, device=dev)
        self.normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self.curvature = torch.empty((n,), dtype=torch.float32, device=dev)
        self.variance = torch.empty((n, 3), dtype=torch.float64, device=dev)
        self.header = torch.empty((8,), dtype=torch.int32, device=dev)
        nbytes = ctypes.c_ulonglong(0)
        pn2._lib.launch("pn2_radius_workspace_size", dev, n, ctypes.byref(nbytes), stream=False)
        self.ws = torch.empty((int(nbytes.value) + 255,), dtype=torch.uint8, device=dev)
        off = (-self.ws.data_ptr()) % 256
        self.view = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        p = pn2._lib.ptr
        self.args = (dev, n, p(points), None, float(radius), 3, self.view, p(self.count), p(self.moments), p(self.normals),
                     p(self.curvature), p(self.variance), p(self.header), self.ws.data_ptr() + off, int(nbytes.value))
        self.keep = points

    def __call__(self):
        pn2._lib.launch("pn2_radius_neighborhoods", *self.args)

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

    def outputs(self):
        return tuple(t.cpu().numpy().tobytes() for t in (self.count, self.moments, self.normals, self.curvature, self.variance,
                                                         self.header))


def parts(call, rounds):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(rounds):
            call()
        torch.cuda.synchronize()
    t = {"grid": 0.0, "scan": 0.0, "header": 0.0, "other": 0.0}
    for ev in prof.events():
        dur = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
        if not dur:
            continue
        name = ev.name
        which = ("grid" if any(k in name for k in GRID) or "adix" in name or "onesweep" in name.lower() else
                 "scan" if "radius_scan" in name else "header" if "radius_header" in name else "other")
        t[which] += dur
    return {k: round(v / rounds / 1e3, 4) for k, v in t.items()}


def host_baseline(points, radius, most):
    """-> seconds (the loop's share scaled from `most` points to all), the counts, the points looped over"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = points.astype(np.float64)
    found = cKDTree(p).query_ball_point(p, float(np.float32(radius)))
    t1 = time.perf_counter()
    say("KD-tree queried")
    some = np.unique(np.linspace(0, len(p) - 1, min(len(p), most)).astype(np.int64))
    for i in some:
        q = p[found[i]]
        if len(q) >= 3:
            np.linalg.eigh(np.cov(q.T, bias=True))
    t2 = time.perf_counter()
    return (t1 - t0) + (t2 - t1) * len(p) / len(some), np.array([len(v) for v in found], dtype=np.int32), len(some)


def variants_ab(raw, spans, alternations, reps):
    dbg = pn2._lib._raw.pn2_debug_set
    settings = [(1, SHIPPED_SPAN)] + [(0, s) for s in spans]
    runs = {s: [] for s in settings}
    want = None
    for _ in range(alternations):
        for variant, span in settings:
            assert dbg(HOOK_VARIANT, variant) == 0 and dbg(HOOK_SPAN, span) == 0
            runs[(variant, span)].append(raw.device_ms(reps))
            got = raw.outputs()
            want = want or got
            assert got == want, "a variant changed the result"
    out = {}
    for (variant, span), r in runs.items():
        assert dbg(HOOK_VARIANT, variant) == 0 and dbg(HOOK_SPAN, span) == 0
        out["lane" if variant else "auto,span=%d" % span] = dict(stats(r), scan_kernel_ms=parts(raw, 3)["scan"])
    assert dbg(HOOK_VARIANT, 0) == 0 and dbg(HOOK_SPAN, SHIPPED_SPAN) == 0  # as the library ships, for what follows
    return out


def case(name, args, dev):
    points, _ = cluster_cost.CASES[name][0]()
    radius = RADIUS[name]
    d_pts = torch.from_numpy(points).to(dev)

    def call():
        return pn2.radius_neighborhoods(d_pts, radius, viewpoint=(0, 0, 0), moments=True, variance=True)

    nb = call()  # the warm-up of every shape timed below
    count = nb.count.cpu().numpy()
    out = {"case": name, "points": len(points), "radius": radius, "valid": nb.valid, "largest_count": int(count.max()),
           "mean_count": round(float(count.mean()), 2), "with_normal": int((count >= 3).sum())}
    say(name, "warm")
    out["call_ms"] = stats([wall_ms(call) for _ in range(args.rounds)])
    raw = Raw(d_pts, radius)
    out["device_ms"] = stats([raw.device_ms(args.reps) for _ in range(args.rounds)])
    try:
        out["parts_ms"] = parts(raw, args.rounds)
    except Exception as err:  # no tracer in this build of torch
        out["parts_ms"], out["parts_error"] = None, repr(err)[:200]
    say("library timed")
    if not args.no_host:
        try:
            seconds, host_count, looped = host_baseline(points, radius, args.host_points)
            # the KD-tree measures in its own arithmetic: a pair exactly on the radius may differ
            out["host_s"], out["host_points_looped"] = round(seconds, 3), looped
            out["host_same_counts"] = bool(np.array_equal(host_count, count))
            out["host_over_call"] = round(seconds * 1e3 / out["call_ms"]["median"], 1)
        except ImportError:
            out["host_s"] = "no baseline: scipy does not import"
        say("host baseline")
    if hasattr(pn2._lib._raw, "pn2_debug_set"):
        out["variants"] = variants_ab(raw, args.spans, args.alternations, args.reps)
        say("variants")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(RADIUS), choices=list(RADIUS))
    ap.add_argument("--host-points", type=int, default=20000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--spans", type=int, nargs="+", default=[0, 1, 2, 4, 8], help="kSpan settings for the tuning build's A/B")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.cases:
        out = case(name, args, dev)
        out["device"], out["library"] = torch.cuda.get_device_name(dev), os.path.basename(pn2._lib.LIB_PATH)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
