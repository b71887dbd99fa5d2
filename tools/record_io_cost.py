"""What reading and writing .ply scenes costs ("Record files"), on 4 M points: one JSON line per step with
  (a) a PLY of 27-byte rows (double x y z + uchar red green blue) and one of 15-byte rows (float x y z + uchar colours), written
      and read: scene_io's device functions against the host functions of util.point_cloud_util, files in the page cache;
  (b) the 16-byte .pcd path (x y z rgb, pn2_pcd_pack / pn2_pcd_unpack) as the yardstick for bytes per second;
  (c) the two record kernels alone on a resident buffer, the staged form against the plain form (PN2_REC_FORM_PLAIN), at the
      strides 15, 27 and 64, from device events.
Every figure is the median of 5 runs in this process after one warm-up run, with the 5 runs beside it: a difference between two
forms counts only where it exceeds their spread.  Every step runs under a time limit of its own: SIGALRM at its default action
ends the process where a step overruns, and nothing is started after it; the lines printed so far stand.
usage: python tools/record_io_cost.py [--points N] [--dir DIR]"""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

launch, ptr, int_array = pn2._lib.launch, pn2._lib.ptr, pn2._lib.int_array
C = pn2._lib.ABI.constants
U = pn2.util.point_cloud_util
PLAIN = C["PN2_REC_FORM_PLAIN"]


def step(name, seconds, fn):
    """fn() under its own time limit -> one JSON line"""
    signal.alarm(seconds)  # default action: the process ends there
    out = fn()
    signal.alarm(0)
    print(json.dumps(dict(step=name, **out)), flush=True)


def wall_ms(fn, reps=5):
    fn()  # warm-up: allocator, pinned buffers, page cache
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(v)), 3), runs=[round(x, 3) for x in v])


def event_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        v.append(s.elapsed_time(e))
    return dict(ms=round(float(np.median(v)), 4), runs=[round(x, 4) for x in v])


def with_rate(t, nbytes):
    t["GB_per_s"] = round(nbytes / t["ms"] / 1e6, 2)
    return t


def files(dev, d, n, points, colors):
    dp, dc = torch.from_numpy(points).to(dev), torch.from_numpy(colors).to(dev)
    for coord, row in (("double", 27), ("float", 15)):
        path_d, path_h = os.path.join(d, "dev_%d.ply" % row), os.path.join(d, "host_%d.ply" % row)
        nbytes = n * row
        step("ply%d_write_device" % row, 120, lambda: with_rate(wall_ms(lambda: pn2.write_point_cloud_ply(path_d, dp, dc, coord=coord)), nbytes))
        step("ply%d_write_host" % row, 240, lambda: with_rate(wall_ms(lambda: U.write_point_cloud_ply(path_h, points, colors, coord=coord)), nbytes))
        with open(path_d, "rb") as a, open(path_h, "rb") as b:
            assert a.read() == b.read()
        step("ply%d_read_device" % row, 120, lambda: with_rate(wall_ms(lambda: pn2.read_point_cloud_ply(path_d, dev)), nbytes))
        step("ply%d_read_host_to_device" % row, 240, lambda: with_rate(
            wall_ms(lambda: [torch.from_numpy(a).to(dev) for a in U.read_point_cloud_ply(path_h)]), nbytes))
    path = os.path.join(d, "yard.pcd")
    step("pcd16_write_device", 120, lambda: with_rate(wall_ms(lambda: pn2.write_point_cloud_pcd(path, dp, dc)), n * 16))
    step("pcd16_read_device", 120, lambda: with_rate(wall_ms(lambda: pn2.read_point_cloud_pcd(path, dev)), n * 16))


def unpack_alone(dev, n, stride, offsets, types, kind):
    """pn2_record_unpack on resident rows, colours written: staged against plain, alternating"""
    rows = pn2.preprocess._aligned((n * stride + 15) // 16 * 16, dev)
    rows.copy_(torch.randint(0, 256, (rows.numel(),), dtype=torch.uint8, device=dev))
    points = torch.empty((n, 3), dtype=torch.float64, device=dev)
    colors = torch.empty((n, 3), dtype=torch.float64, device=dev)
    off_a, type_a = int_array(offsets), int_array(types)
    call = lambda form: launch("pn2_record_unpack", dev, ptr(rows), n, stride, off_a, type_a, kind, form, ptr(points), ptr(colors),  # noqa: E731
                               None, None)
    out, keep = {}, {}
    for name, form in (("staged", 0), ("plain", PLAIN), ("staged_again", 0)):
        out[name] = with_rate(event_ms(lambda: call(form)), n * (stride + 48))
        keep[name] = (points.clone(), colors.clone())
    same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(keep["staged"], keep["plain"]))
    return dict(n=n, stride=stride, same_bits=same, **out)


def pack_alone(dev, n, coord, stride):
    points = torch.randn((n, 3), dtype=torch.float64, device=dev)
    colors = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
    rows = pn2.preprocess._aligned(n * stride, dev)
    call = lambda form: launch("pn2_record_pack", dev, ptr(points), C["PN2_PCD_F64"], ptr(colors), C["PN2_PCD_COLOR_U8"], None, n,  # noqa: E731
                               C["PN2_REC_F64" if coord == "double" else "PN2_REC_F32"], form, ptr(rows))
    out, keep = {}, {}
    for name, form in (("staged", 0), ("plain", PLAIN), ("staged_again", 0)):
        out[name] = with_rate(event_ms(lambda: call(form)), n * (stride + 27))
        keep[name] = rows.clone()
    return dict(n=n, stride=stride, same_bits=torch.equal(keep["staged"], keep["plain"]), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.points
    rs = np.random.RandomState(0)
    points = rs.uniform(-100, 100, (n, 3))
    colors = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    print(json.dumps(dict(step="setup", points=n, device=torch.cuda.get_device_name(dev))), flush=True)
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        files(dev, d, n, points, colors)
    f32, f64, u8 = C["PN2_REC_F32"], C["PN2_REC_F64"], C["PN2_REC_U8"]
    three = C["PN2_REC_COLOUR_THREE"]
    layouts = {15: ([0, 4, 8, 12, 13, 14, -1], [f32] * 3 + [u8] * 4), 27: ([0, 8, 16, 24, 25, 26, -1], [f64] * 3 + [u8] * 4),
               64: ([0, 8, 16, 24, 25, 26, -1], [f64] * 3 + [u8] * 4)}
    for stride, (offsets, types) in layouts.items():
        step("unpack_alone_%d" % stride, 60, lambda: unpack_alone(dev, n, stride, offsets, types, three))
    for coord, stride in (("float", 15), ("double", 27)):
        step("pack_alone_%d" % stride, 60, lambda: pack_alone(dev, n, coord, stride))


if __name__ == "__main__":
    main()
