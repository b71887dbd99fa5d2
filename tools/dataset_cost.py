"""What the multi-scene SemanticDataset costs ("Multi-scene dataset"): one JSON line with
  (a) one SemanticDataset.sample_batch_in_all_files batch (B=16, N=8192, augment=True) on the synthetic store of
      examples/train_semantic3d.py (columns of 50k+ points), eager calls back to back and as a replayed one-call graph;
  (b) today's single-scene path at the same column sizes: SemanticFileData.sample_batch on the largest scene of that store
      plus the examples' torch.cat of coordinates and colours and the label-weight gather;
  (c) the captured training step fed by the dataset through the prefetch path (next batch sampled on a side stream) against
      the same step on a resident batch.
Every figure is the median of 5 regions (20 calls / steps each).  usage: python tools/dataset_cost.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import pn2_amd as pn2  # noqa: E402
import train_semantic3d as ex  # noqa: E402


def region_ms(fn, k=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def med(fn, k=20, reps=5):
    v = [region_ms(fn, k) for _ in range(reps)]
    return round(float(np.median(v)), 4), [round(x, 4) for x in v]


def main():
    dev = torch.device("cuda:0")
    B, N = 16, 8192
    out = {"B": B, "N": N}
    scenes = {k: ex.synthetic_scene(*v) + (k,) for k, v in ex.SYNTHETIC.items()}
    train = [scenes[k] for k in ex.SYNTHETIC_SPLITS["train"]]
    ds = pn2.dataset.SemanticDataset(N, "train", True, 10, 10, "", device=dev, seed=0, scenes=train)

    # ---- (a) the new path
    ds.sample_batch_in_all_files(B)
    torch.cuda.synchronize()
    out["a_column_points"] = sorted(ds.last_cnt.cpu().tolist())
    out["a_batch_ms"], out["a_regions"] = med(lambda: ds.sample_batch_in_all_files(B))
    ds.check_last()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            ds.sample_batch_in_all_files(B)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    out["a_graph_replay_ms"], _ = med(g.replay)
    out["a_launches_per_batch"] = 4  # ds_count, ds_select, ds_emit, ds_write (csrc/pn2_dataset.hip)

    # ---- (b) the single-scene path of the examples, on the largest scene
    p, lab, col, _ = train[0]
    fd = pn2.dataset.SemanticFileData(points=p, labels=lab, colors=col, box_size_x=10, box_size_y=10, device=dev)
    lw = torch.from_numpy(ds.label_weights).float().to(dev)

    def single():
        c, _, lb, cl = fd.sample_batch(B, N, capacity=131072)
        return torch.cat([c, cl], dim=2), lb.long(), lw[lb.long()]
    single()
    out["b_column_points"] = sorted(fd.last_cnt.cpu().tolist())
    out["b_batch_ms"], out["b_regions"] = med(single)
    fd.check_last()

    # ---- (c) the captured training step: fed by the dataset through the prefetch path vs a resident batch
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    side = torch.cuda.Stream()
    fed = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev)
    res = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev)
    cur = [ds.sample_batch_in_all_files(B)]
    resident = [ds.sample_batch_in_all_files(B), ds.sample_batch_in_all_files(B)]
    count = [0]

    def fed_step():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            nxt = ds.sample_batch_in_all_files(B)
        torch.cuda.current_stream().wait_stream(side)
        for t in nxt:
            t.record_stream(torch.cuda.current_stream())
        fed.train_step(*cur[0], sync=False, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2])
        cur[0] = nxt

    def res_step():
        i = count[0]
        count[0] += 1
        a, b = resident[i % 2], resident[(i + 1) % 2]
        res.train_step(*a, sync=False, next_pc=b[0], next_labels=b[1], next_smpw=b[2])
    for _ in range(7):
        fed_step()
        res_step()
    f, r = [], []
    for _ in range(5):
        f.append(region_ms(fed_step))
        r.append(region_ms(res_step))
    out["c_step_ms_dataset_fed"] = round(float(np.median(f)), 4)
    out["c_step_ms_resident"] = round(float(np.median(r)), 4)
    out["c_regions_fed"] = [round(v, 4) for v in f]
    out["c_regions_resident"] = [round(v, 4) for v in r]
    ds.check_last()
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
