"""What parsing a raw Semantic3D scan costs: one JSON line, measurements and no thresholds.
On a generated <lines>-line .txt (`%.3f %.3f %.3f %d %d %d %d`, 1 intensity in 50 a non-integer; about 39 bytes per line):
  (a) the kernels alone on resident text: pn2_text_index_lines, pn2_text_parse and both, device events around regions of
      --calls back-to-back calls, in GB/s of text, and the bytes they move (the text three times -- count, starts, parse --, the
      line index written once and read once, 41 bytes of output per line) against the achievable HBM rate;
  (b) end to end, pn2.parse_text on the file in the page cache (read once before), host clock around a device synchronise, next to
      the pinned-copy rate and the file -> pinned-buffer read rate measured in the same run;
  (c) the host baseline on --baseline-lines lines: the reference's per-line loop (preprocess.py:40-46: split, int(float(tokens[3])),
      join, write) and util.point_cloud_util.load_labels, scaled to <lines>.  The baseline is the comparison, never the code under test.
Every figure: the median of --regions regions after a warm-up, with the smallest and the largest.
usage: python tools/text_parse_cost.py [--lines 10000000] [--regions 7] [--calls 10] [--baseline-lines 1000000]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402

P = pn2.preprocess
L = pn2._lib
HBM_ACHIEVABLE = 6.3e12  # bytes/s, float4 copy on the MI355X


def spread(values, digits=3):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def write_scan(path, lines, label_path=None):
    """-> bytes written.  Blocks of 10^6 lines, each from its own seed."""
    with open(path, "w") as f, open(label_path or os.devnull, "w") as lf:
        for block, start in enumerate(range(0, lines, 1000000)):
            n = min(1000000, lines - start)
            rs = np.random.RandomState(7000 + block)
            xyz = (rs.uniform(-300, 300, (n, 3)) * rs.uniform(0, 1, (n, 1))).tolist()
            inten = rs.randint(-2047, 2048, n).tolist()
            rgb = rs.randint(0, 256, (n, 3)).tolist()
            f.write("".join("%.3f %.3f %.3f %s %d %d %d\n" % (x, y, z, i if k % 50 else "%.1f" % (i + 0.5), r, g, b)
                            for k, ((x, y, z), i, (r, g, b)) in enumerate(zip(xyz, inten, rgb))))
            lf.write("".join("%d\n" % v for v in rs.randint(0, 9, n).tolist()))
            print("generated %d lines" % (start + n), file=sys.stderr, flush=True)
    return os.path.getsize(path)


def kernels_alone(path, nbytes, args, dev, out):
    with open(path, "rb") as f:
        text = P._aligned(nbytes, dev)
        text.copy_(torch.frombuffer(bytearray(f.read()), dtype=torch.uint8))
    starts = P.index_lines(text)
    n = starts.numel() - 1
    cap = n + 1
    need = L.u64_array([0])
    L.launch("pn2_text_index_workspace_bytes", dev, nbytes, need, stream=False)
    ws = P._aligned(int(need[0]), dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    f64 = torch.empty((n, 3), dtype=torch.float64, device=dev)
    i32 = torch.empty((n, 4), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    status = torch.empty((3,), dtype=torch.int32, device=dev)
    kinds = L.int_array(P.SEMANTIC3D_KINDS)

    def index():
        L.launch("pn2_text_index_lines", dev, L.ptr(text), nbytes, L.ptr(starts), cap, L.ptr(count), L.ptr(ws), ws.numel())

    def parse():
        L.launch("pn2_text_parse", dev, L.ptr(text), nbytes, L.ptr(starts), n, kinds, len(kinds), L.ptr(f64), L.ptr(i32),
                 L.ptr(flags), L.ptr(status))

    def both():
        index()
        parse()

    moved = dict(index=2 * nbytes + 4 * (n + 1), parse=nbytes + 4 * (n + 1) + 41 * n)  # bytes to and from HBM, by construction
    moved["both"] = moved["index"] + moved["parse"]
    for name, fn in (("index", index), ("parse", parse), ("both", both)):
        for _ in range(2 * args.calls):
            fn()
        ms = []
        for _ in range(args.regions):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.calls)
        out["kernels_%s_ms" % name] = spread(ms)
        out["kernels_%s_text_GBps" % name] = spread([nbytes / (m * 1e-3) / 1e9 for m in ms], 1)
        med = sorted(ms)[len(ms) // 2]
        out["kernels_%s_moved_bytes" % name] = moved[name]
        out["kernels_%s_fraction_of_achievable_hbm" % name] = round(moved[name] / (med * 1e-3) / HBM_ACHIEVABLE, 4)
    assert status.tolist()[1:] == [0, 0] and int(count.item()) == n
    out["lines"] = n


def end_to_end(path, nbytes, args, dev, out):
    chunk = 256 << 20
    pinned = torch.empty((min(chunk, nbytes),), dtype=torch.uint8).pin_memory()
    device = torch.empty_like(pinned, device=dev)
    view = memoryview(pinned.numpy())
    copy_GBps, read_GBps, parse_s = [], [], []
    for k in range(args.regions + 1):  # the first region of each is the warm-up (page cache, allocator, code objects)
        with open(path, "rb", buffering=0) as f:
            t0 = time.perf_counter()
            got = 0
            while got < len(view):
                got += f.readinto(view[got:])
            t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        device.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        f64, i32, stats = P.parse_text(path, P.SEMANTIC3D_KINDS, device=dev, chunk_bytes=chunk)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        del f64, i32
        if k:
            read_GBps.append(len(view) / (t1 - t0) / 1e9)
            copy_GBps.append(len(view) / (t3 - t2) / 1e9)
            parse_s.append(t4 - t3)
    out["end_to_end_s"] = spread(parse_s)
    out["end_to_end_text_GBps"] = spread([nbytes / s / 1e9 for s in parse_s], 2)
    out["pinned_copy_GBps"] = spread(copy_GBps, 1)
    out["file_to_pinned_read_GBps"] = spread(read_GBps, 2)
    out["end_to_end_chunks"], out["end_to_end_slow_tokens"] = stats.chunks, stats.slow_tokens


def host_baseline(tmp, args, out):
    txt, labels = os.path.join(tmp, "baseline.txt"), os.path.join(tmp, "baseline.labels")
    write_scan(txt, args.baseline_lines, labels)
    scale = args.lines / args.baseline_lines
    loop_s, labels_s = [], []
    for k in range(args.regions + 1):
        t0 = time.perf_counter()
        with open(txt, "r") as src, open(os.path.join(tmp, "baseline.pts"), "w") as dst:
            for line in src:  # what preprocess.py:40-46 does to every line
                fields = line.split()
                fields[3] = str(int(float(fields[3])))
                dst.write(" ".join(fields) + "\n")
        t1 = time.perf_counter()
        got = pn2.util.point_cloud_util.load_labels(labels)
        t2 = time.perf_counter()
        assert len(got) == args.baseline_lines
        if k:
            loop_s.append((t1 - t0) * scale)
            labels_s.append((t2 - t1) * scale)
    out["baseline_lines_timed"] = args.baseline_lines
    out["baseline_txt_loop_s_scaled"] = spread(loop_s, 2)
    out["baseline_load_labels_s_scaled"] = spread(labels_s, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--baseline-lines", type=int, default=1000000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_parse_cost needs the MI355X: a CPU run gives no rate")
    dev = torch.device("cuda:0")
    out = dict(tool="text_parse_cost", device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scan.txt")
        labels = os.path.join(tmp, "scan.labels")
        nbytes = write_scan(path, args.lines, labels)
        out["text_bytes"] = nbytes
        kernels_alone(path, nbytes, args, dev, out)
        end_to_end(path, nbytes, args, dev, out)
        t = []
        for k in range(args.regions + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = pn2.load_labels(labels, dev)
            torch.cuda.synchronize()
            if k:
                t.append(time.perf_counter() - t0)
        assert got.numel() == args.lines
        out["load_labels_s"] = spread(t)
        host_baseline(tmp, args, out)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
