"""What writing and reading the scene files of the predict flow costs: one JSON line, measurements and no
thresholds.
  (a) the integer formatter alone on resident values: pn2_text_format_i32, device events around regions of --calls back-to-back
      calls, for 10^7 and 10^8 single-digit labels (the latter in two calls: one call takes at most PN2_TEXT_MAX_BYTES / 12
      tokens) and 10^7 rows of 4 columns of mixed width; the bytes it moves (the values read by both passes, the text written once)
      against the achievable HBM rate;
  (b) pn2.write_labels, pn2.write_point_cloud_pcd and pn2.read_point_cloud_pcd at --points points, files in the page cache, host
      clock around a device synchronise, next to the host functions of util/point_cloud_util.py timed in the same run on the same
      host (pn2.load_labels against the host load_labels as well: the example reads the dense ground truth with it).  The
      baseline is the host functions, never the code under test;
  (c) with --parent-tree PATH (a built checkout of the parent commit): examples/predict_semantic3d.py on one synthetic scene of
      --points points as a process of its own, this tree and the parent's in turn, wall time of the process.
Every figure: the median of --regions regions after a warm-up, with the smallest and the largest.
usage: python tools/scene_io_cost.py [--points 4000000] [--regions 5] [--calls 10] [--parent-tree PATH] [--only-formatter]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

L = pn2._lib
S = pn2.scene_io
U = pn2.util.point_cloud_util
HBM_ACHIEVABLE = 6.3e12  # bytes/s, float4 copy on the MI355X


def spread(values, digits=3):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def formatter_alone(name, values, args, dev, out):
    """values: (n, ncols) int32 on the device, formatted in calls of at most the ABI's range"""
    n, ncols = values.shape
    per_call = min(n, S.MAX_TEXT_BYTES // (S.I32_CHARS * ncols))
    parts = [values[lo:lo + per_call] for lo in range(0, n, per_call)]
    fmt = S._Formatter(per_call, ncols, dev)
    tiny = pn2.preprocess._aligned(16, dev)
    texts, need = [], 0
    for part in parts:  # text_cap = 0: nothing is written, *out_bytes is what the rows need
        L.launch("pn2_text_format_i32", dev, L.ptr(part), part.shape[0], ncols, L.ptr(tiny), 0, L.ptr(fmt.out_bytes), L.ptr(fmt.ws),
                 fmt.ws.numel())
        texts.append(pn2.preprocess._aligned(int(fmt.out_bytes.item()), dev))
        need += texts[-1].numel()

    def call():
        for part, text in zip(parts, texts):
            fmt(part, text)

    for _ in range(args.calls):
        call()
    ms = []
    for _ in range(args.regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / args.calls)
    moved = 2 * 4 * n * ncols + need  # bytes to and from HBM, by construction
    med = sorted(ms)[len(ms) // 2]
    out["format_%s" % name] = dict(rows=n, ncols=ncols, calls_per_table=len(parts), text_bytes=need, ms=spread(ms),
                                   text_GBps=spread([need / (m * 1e-3) / 1e9 for m in ms], 1), moved_bytes=moved,
                                   fraction_of_achievable_hbm=round(moved / (med * 1e-3) / HBM_ACHIEVABLE, 4))
    # the text is the host's for the first rows
    head = values[:1000].cpu().numpy()
    want = b"".join(b" ".join(b"%d" % v for v in row) + b"\n" for row in head.tolist())
    assert texts[0][:len(want)].cpu().numpy().tobytes() == want
    print("formatter %s: %s" % (name, json.dumps(out["format_%s" % name])), file=sys.stderr, flush=True)


def timed(fn, regions, sync=True):
    t = []
    for k in range(regions + 1):  # the first region is the warm-up (page cache, allocator, code objects)
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if k:
            t.append(time.perf_counter() - t0)
    print("timed %s" % spread(t, 4), file=sys.stderr, flush=True)
    return spread(t, 4)


def files(tmp, args, dev, out):
    n = args.points
    rs = np.random.RandomState(5)
    labels_h = rs.randint(0, 9, n).astype(np.int32)
    points_h = (rs.uniform(-300, 300, (n, 3))).astype(np.float32)
    colors_h = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    unit_h = colors_h.astype(np.float64) / 255.0
    labels, points, colors = (torch.from_numpy(a).to(dev) for a in (labels_h, points_h, colors_h))
    p = lambda name: os.path.join(tmp, name)  # noqa: E731
    res = out["files"] = dict(points=n)
    res["write_labels_device_s"] = timed(lambda: pn2.write_labels(p("d.labels"), labels), args.regions)
    res["write_labels_host_s"] = timed(lambda: U.write_labels(p("h.labels"), labels.cpu().numpy()), args.regions)
    res["write_pcd_device_s"] = timed(lambda: pn2.write_point_cloud_pcd(p("d.pcd"), points, colors), args.regions)
    res["write_pcd_host_s"] = timed(lambda: U.write_point_cloud_pcd(p("h.pcd"), points.cpu().numpy(), colors.cpu().numpy().astype(
        np.float64) / 255.0), args.regions)
    res["read_pcd_device_s"] = timed(lambda: pn2.read_point_cloud_pcd(p("d.pcd"), dev), args.regions)
    res["read_pcd_host_s"] = timed(lambda: U.read_point_cloud_pcd(p("h.pcd")), args.regions, sync=False)
    res["load_labels_device_s"] = timed(lambda: pn2.load_labels(p("d.labels"), dev), args.regions)
    res["load_labels_host_s"] = timed(lambda: U.load_labels(p("h.labels")), args.regions, sync=False)
    for a, b in (("d.labels", "h.labels"), ("d.pcd", "h.pcd")):
        with open(p(a), "rb") as fa, open(p(b), "rb") as fb:
            assert fa.read() == fb.read(), a
    got_p, got_c = pn2.read_point_cloud_pcd(p("d.pcd"), dev)
    assert np.array_equal(got_p.cpu().numpy(), points_h.astype(np.float64)) and np.array_equal(got_c.cpu().numpy(), unit_h)
    for k in ("write_labels", "write_pcd", "read_pcd", "load_labels"):
        res[k + "_host_over_device"] = round(res[k + "_host_s"]["median"] / res[k + "_device_s"]["median"], 2)


def example_scene(tmp, args, out):
    trees = [("this", ROOT), ("parent", os.path.abspath(args.parent_tree))]
    cmd = ["--scenes", "1", "--scene-points", str(args.points), "--num_samples", str(args.samples)]
    wall = {name: [] for name, _ in trees}
    for k in range(args.regions + 1):
        for name, tree in trees:  # in turn: both see the same state of the host
            t0 = time.perf_counter()
            run = subprocess.run([sys.executable, os.path.join(tree, "examples", "predict_semantic3d.py"), "--out",
                                  os.path.join(tmp, "result_" + name)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp)
            dt = time.perf_counter() - t0
            if run.returncode != 0:
                raise SystemExit("%s: examples/predict_semantic3d.py failed:\n%s" % (name, run.stdout.decode(errors="replace")[-2000:]))
            if k:
                wall[name].append(dt)
            print("example: region %d, %s tree %.2f s" % (k, name, dt), file=sys.stderr, flush=True)
    differ = []  # did both trees write the same files?
    for sub in ("sparse", "dense"):
        for fname in sorted(os.listdir(os.path.join(tmp, "result_this", sub))):
            with open(os.path.join(tmp, "result_this", sub, fname), "rb") as fa, open(os.path.join(tmp, "result_parent", sub, fname), "rb") as fb:
                if fa.read() != fb.read():
                    differ.append(sub + "/" + fname)
    out["example_one_scene"] = dict(points=args.points, samples=args.samples, this_commit_wall_s=spread(wall["this"], 2),
                                    parent_commit_wall_s=spread(wall["parent"], 2), files_that_differ=differ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: adds measurement (c)")
    ap.add_argument("--only-formatter", action="store_true", help="measurement (a) alone (PN2_HIP_LIBRARY=...: another build)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_io_cost needs the MI355X: a CPU run gives no rate")
    dev = torch.device("cuda:0")
    out = dict(tool="scene_io_cost", device=torch.cuda.get_device_name(0))
    g = torch.Generator(device=dev).manual_seed(1)
    formatter_alone("labels_1e7", torch.randint(0, 9, (10 ** 7, 1), generator=g, device=dev, dtype=torch.int32), args, dev, out)
    formatter_alone("labels_1e8", torch.randint(0, 9, (10 ** 8, 1), generator=g, device=dev, dtype=torch.int32), args, dev, out)
    width = 10 ** torch.randint(0, 10, (10 ** 7, 4), generator=g, device=dev)  # a magnitude class per token, then a value in it
    mixed = torch.fmod(torch.randint(-2 ** 31, 2 ** 31, (10 ** 7, 4), generator=g, device=dev), width).to(torch.int32)  # both signs
    formatter_alone("mixed_1e7x4", mixed, args, dev, out)
    del width, mixed
    torch.cuda.empty_cache()
    if args.only_formatter:
        print(json.dumps(out))
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        files(tmp, args, dev, out)
        if args.parent_tree:
            example_scene(tmp, args, out)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
