"""What building the SemanticDataset store costs ("Store ingest"): one JSON line with the constructor's
wall time up to and including a resident store (the host path's first _upload included), ingest="host" against
ingest="device", on
  (a) the synthetic training store of examples/train_semantic3d.py (2.8 M points in 3 scenes), taken from host arrays;
  (b) the same scenes from .pcd / .labels files in the page cache (written once, read once before the clock starts);
and the ingest call alone at n = 1.5 M (the largest of those scenes): the whole call from events, and its key kernel, its sort
and its gather from the device times torch's profiler records per kernel.
Every figure is the median of 5 runs in this process (the parts: the mean of 5 calls).  usage: python tools/ingest_cost.py [--dir DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import pn2_amd as pn2  # noqa: E402
import train_semantic3d as ex  # noqa: E402

launch, ptr, u64_array = pn2._lib.launch, pn2._lib.ptr, pn2._lib.u64_array

N = 8192


def wall_ms(fn, reps=5):
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(v)), 3), [round(x, 3) for x in v]


def resident(dev, ingest, **kw):
    """the constructor, up to and including a store in HBM"""
    ds = pn2.dataset.SemanticDataset(N, "train", True, 10, 10, kw.pop("path", ""), device=dev, seed=0, ingest=ingest, **kw)
    ds._upload(16)
    return ds


def ingest_alone(dev, pts, labels, cols, out):
    """the raw call on one scene already in HBM: the whole call from events, its parts from the profiler"""
    n = len(pts)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    p, c, lab = t(pts, np.float64), t(cols, np.float64), t(labels, np.int32)
    o_p, o_c = torch.empty_like(p), torch.empty((n, 3), dtype=torch.float32, device=dev)
    o_l, o_perm = torch.empty((n,), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    res = torch.empty((12,), dtype=torch.int64, device=dev)
    nbytes = u64_array([0])
    launch("pn2_scene_ingest_workspace_size", dev, n, nbytes, stream=False)
    ws = torch.empty((int(nbytes[0]) + 256,), dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 256:]

    def call():
        launch("pn2_scene_ingest", dev, n, ptr(p), ptr(c), ptr(lab), ptr(o_p), ptr(o_c), ptr(o_l), ptr(o_perm), ptr(res[0:2]),
               ptr(res[2:11]), ptr(res[11:12]), ptr(ws), ws.numel())
    call()
    torch.cuda.synchronize()
    assert int(res[11:12].view(torch.int32)[0]) == 0
    times = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        call()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    out["ingest_n"] = n
    out["ingest_call_ms"] = round(float(np.median(times)), 4)
    out["ingest_call_runs"] = [round(x, 4) for x in times]
    # the parts: device time per kernel of 5 more calls from torch's profiler, by kernel name (the sort is whatever is neither
    # one of the library's three kernels nor a memset); the median call's share each
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                call()
            torch.cuda.synchronize()
        parts = {"key": [], "sort": [], "gather": [], "finish": [], "memset": []}
        for ev in prof.events():
            name = ev.name
            which = ("key" if "ingest_key" in name else "gather" if "ingest_gather" in name else "finish" if "ingest_finish" in name
                     else "memset" if "emset" in name else "sort")
            dur = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
            if dur:
                parts[which].append(dur)
        out["ingest_parts_ms"] = {k: round(sum(v) / 5 / 1e3, 4) for k, v in parts.items()}
        out["ingest_parts_launches"] = {k: len(v) // 5 for k, v in parts.items()}
    except Exception as err:  # no tracer in this build of torch: the whole call above stands alone
        out["ingest_parts_ms"] = None
        out["ingest_parts_error"] = repr(err)[:200]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the scene files of (b) are written (default: a temporary directory)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    scenes = [ex.synthetic_scene(*ex.SYNTHETIC[k]) + (k,) for k in ex.SYNTHETIC_SPLITS["train"]]
    out["points"] = [len(s[0]) for s in scenes]
    out["x_ties"] = [int(len(s[0]) - len(np.unique(s[0][:, 0]))) for s in scenes]
    resident(dev, "device", scenes=scenes)  # warm-up: library, allocator, pinned buffers

    out["a_host_ms"], out["a_host_runs"] = wall_ms(lambda: resident(dev, "host", scenes=scenes))
    out["a_device_ms"], out["a_device_runs"] = wall_ms(lambda: resident(dev, "device", scenes=scenes))
    on = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in s[:3]) + (s[3],) for s in scenes]
    out["a_device_from_hbm_ms"], out["a_device_from_hbm_runs"] = wall_ms(lambda: resident(dev, "device", scenes=on))
    del on

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for p, lab, c, name in scenes:
            pn2.scene_io.write_point_cloud_pcd(os.path.join(d, name + ".pcd"), p, c)
            pn2.scene_io.write_labels(os.path.join(d, name + ".labels"), lab)
        splits = {"train": [s[3] for s in scenes]}
        resident(dev, "device", path=d, splits=splits)  # the files are in the page cache from here on
        out["b_host_ms"], out["b_host_runs"] = wall_ms(lambda: resident(dev, "host", path=d, splits=splits))
        out["b_device_ms"], out["b_device_runs"] = wall_ms(lambda: resident(dev, "device", path=d, splits=splits))

    ingest_alone(dev, *scenes[0][:3], out)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
