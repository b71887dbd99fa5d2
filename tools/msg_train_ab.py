"""Forward + backward of the configs[2] MSG set-abstraction module in TRAINING (B=16, N=8192, M=1024, 64 feature channels; radii /
K / MLPs of benchlib/configs.py other_configs), geometry computed ahead by msg_geometry: the hoisted path
(tf_util.USE_HOISTED_MSG_TRAIN) against the same call with the flag off -- the grouped path, which is the code before the hoisted
path existed.  Each variant is captured into one graph on one stream and replayed (the method of tools/lin_ab.py: fps_ab.timeit
over 20 replays), five rounds, median.  Also prints the library launches of one eager forward + backward (the torch ops of the
grouped path -- cat, amax, the sum of the scales' gradients -- are not library launches and are not counted).
usage: python tools/msg_train_ab.py"""
import collections, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import pn2_amd as pn2
from fps_ab import timeit
from conftest import s_scene
dev = torch.device("cuda:0")
B, N, M, C = 16, 8192, 1024, 64
radii, ks, mlps = [0.25, 0.5, 1.0], [16, 32, 64], [[32, 32, 64], [64, 64, 128], [64, 96, 128]]
tfu, pu, L = pn2.util.tf_util, pn2.util.pointnet_util, pn2._lib
xyz = torch.from_numpy(s_scene(5000, B, N)).to(dev)
g = torch.Generator().manual_seed(0)
pts = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
dy = torch.randn(B, M, sum(m[-1] for m in mlps), generator=g).to(dev)
geo = pu.msg_geometry(xyz, M, radii, ks)
store = tfu.set_default_store(tfu.VariableStore(device=dev, seed=1))


def step():
    tfu.reset_bn_links()
    _, out = pu.pointnet_sa_module_msg(xyz, pts, M, radii, ks, mlps, True, 0.5, "msg", geometry=geo)
    out.backward(dy)
    return out


res = {}
for hoisted in (True, False, True, False):  # each variant twice, interleaved: a drift of the machine shows as a spread
    tfu.USE_HOISTED_MSG_TRAIN = hoisted
    for _ in range(2):
        step()
    pts.grad = None
    for p in store.parameters():
        p.grad = None
    L.lib.trace = []
    step()
    torch.cuda.synchronize()
    names = collections.Counter(t[0] for t in L.lib.trace)
    L.lib.trace = None
    pts.grad = None
    for p in store.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    rounds = sorted(timeit(graph.replay, 20) for _ in range(5))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(pts.grad).all())
    res.setdefault(hoisted, []).append(rounds[2])
    print("hoisted=%-5s fwd+bwd (graph replay): median %.1f us (rounds %s); library launches %d: %s"
          % (hoisted, rounds[2], " ".join("%.1f" % r for r in rounds), sum(names.values()),
             ", ".join("%s x%d" % kv for kv in sorted(names.items()))))
    del graph
tfu.USE_HOISTED_MSG_TRAIN = True
on, off = float(np.median(res[True])), float(np.median(res[False]))
print("configs[2] MSG training module: hoisted %.1f us, flag off %.1f us, ratio off/on %.3f" % (on, off, off / on))
