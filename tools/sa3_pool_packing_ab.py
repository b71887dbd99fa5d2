"""The pooled last layer of SA3 (rows x 128 -> 256, relu, max over K = 32): pn2_linear on all rows against
pn2_linear_pool_packed on the live ball-query rows, on the level-3 geometry of the benchmark's inputs at b = 4 / 8 / 16
(8192 / 16384 / 32768 rows).  Both forms read the same H (random source rows gathered through idx: the rows behind a padded
index entry are copies, as behind the chain kernel); interleaved pairs, each timing = 30 launches in one hipGraph replayed three
times.  Prints every pair: the route threshold (pointnet_util.POOL_PACKED_MIN_ROWS) is the smallest size at which the packed
form is faster in every pair."""
import argparse, os, sys, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import pn2_amd as pn2  # noqa: E402
import sa_row_packing_stats as stats  # noqa: E402
from benchlib import inputs as bench_inputs  # noqa: E402


def timeit(fn, iters=30):
    """kernel time, not launch time: `iters` calls captured into one hipGraph, replayed three times (tools/wide_ab.py)"""
    for _ in range(2): fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for _ in range(iters): fn()
        g.replay(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st); g.replay(); g.replay(); g.replay(); e.record(st); torch.cuda.synchronize()
    return s.elapsed_time(e) / (3 * iters) * 1e3



ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--cout", type=int, default=256)
args = ap.parse_args()
tfu, pu, hp = pn2.util.tf_util, pn2.util.pointnet_util, pn2.model.SEMANTIC_HYPERPARAMS
dev = torch.device("cuda:0")
CASES = (("s_scene", 4), ("s_scene", 8), ("s_scene", 16), ("s_dup25", 16), ("s_randn", 16), ("s_randn", 8))
for gen, b in CASES if not os.environ.get("PN2_AB_SHORT") else (CASES[0], CASES[2], CASES[4]):
    pc = torch.from_numpy(getattr(bench_inputs, gen)(0, b, 8192)).to(dev)
    xyz = pc[:, :, 0:3].contiguous()
    with torch.no_grad():
        for lvl in (1, 2, 3):
            src_xyz = xyz
            xyz, idx = pu.sa_geometry(xyz, hp["l%d_npoint" % lvl], hp["l%d_radius" % lvl], hp["l%d_nsample" % lvl])
    groups = idx.shape[0] * idx.shape[1]
    src = torch.randn(b, src_xyz.shape[1], 128, device=dev)
    h = src[torch.arange(b, device=dev)[:, None, None], idx.long()].reshape(groups * 32, 128).contiguous()
    w = torch.randn(128, args.cout, device=dev) / 128 ** 0.5
    bias = 0.1 * torch.randn(args.cout, device=dev)
    plain = lambda: tfu.hip_linear(h, w, bias, relu=True, pool=32)
    packed = lambda: tfu.hip_linear_pool_packed(h, idx, w, bias)
    same = torch.equal(plain().view(torch.int32), packed().view(torch.int32))
    cls = stats.classes(idx.cpu().numpy().reshape(-1, 32))
    blk = min(64, max(8, -(-groups * (args.cout // 64) // 256)))  # pn2_linear_pool_packed's block
    pairs = [(timeit(plain, 30), timeit(packed, 30)) for _ in range(args.pairs)]
    print("%-8s b %2d rows %6d  block %2d  tiles %.2f of un-packed  same bits %s  pairs (pn2_linear, packed) us: %s  packed faster in %d of %d"
          % (gen, b, groups * 32, blk, stats.packed_tiles(cls, blk) / groups, same,
             "  ".join("%.1f %.1f" % p for p in pairs), sum(p[1] < p[0] for p in pairs), len(pairs)), flush=True)
