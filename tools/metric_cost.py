"""What the on-device metrics cost ("Metrics"): one JSON line with
  * pn2_confusion_update on 131072 x 9 logits, timed as a one-node graph replayed back to back (median of 5 regions);
  * the captured training step (B=16, N=8192, semantic.json, staged next batch as in bench.py) with track_metrics on and off,
    median of 5 regions of 20 steps each, the two trainers' regions interleaved;
  * Trainer.eval_step per B=16 batch once it replays its graph (median of 5 regions of 20 batches).
usage: python tools/metric_cost.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402
from benchlib.inputs import s_scene  # noqa: E402


def region_ms(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def main():
    dev = torch.device("cuda:0")
    out = {}
    # ---- the kernel alone
    rs = np.random.RandomState(0)
    C, rows = 9, 131072
    z = torch.from_numpy(rs.randn(rows, C).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rs.randint(0, C, rows).astype(np.int64)).to(dev)
    cm = pn2.util.metric.ConfusionMatrix(C, device=dev)
    loss = torch.ones((), dtype=torch.float32, device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pn2.util.metric.confusion_update(z, lab, confusion=cm.matrix_tensor, invalid=cm.invalid_tensor, loss=loss, loss_acc=acc)
    for _ in range(5):
        g.replay()
    out["kernel_us_131072x9"] = round(float(np.median([region_ms(g.replay, 200) for _ in range(5)])) * 1e3, 2)
    assert int(cm.counts[:C * C].sum()) == rows * (5 + 5 * 200)

    # ---- the training step with and without metrics
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    B, N = 16, 8192
    pc = torch.from_numpy(np.concatenate([s_scene(3000, B, N), rs.random_sample((B, N, 3)).astype(np.float32)], 2)).to(dev)
    labels = torch.from_numpy(rs.randint(0, 9, (B, N)).astype(np.int64)).to(dev)
    smpw = torch.from_numpy((rs.random_sample((B, N)) + 0.5).astype(np.float32)).to(dev)
    pcs = [pc, pc.clone()]
    trainers = {k: pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev, track_metrics=k)
                for k in (True, False)}
    count = {True: 0, False: 0}

    def step(k, sync=False):
        i = count[k]
        count[k] += 1
        return trainers[k].train_step(pcs[i % 2], labels, smpw, next_pc=pcs[(i + 1) % 2], next_labels=labels, next_smpw=smpw,
                                      sync=sync)
    for k in (True, False):
        for _ in range(7):
            step(k, sync=True)
    on, off = [], []
    for _ in range(5):
        on.append(region_ms(lambda: step(True), 20))
        off.append(region_ms(lambda: step(False), 20))
    out["train_step_ms_metrics_on"] = round(float(np.median(on)), 4)
    out["train_step_ms_metrics_off"] = round(float(np.median(off)), 4)
    out["train_step_regions_on"] = [round(v, 4) for v in on]
    out["train_step_regions_off"] = [round(v, 4) for v in off]
    m = trainers[True].train_metrics()
    out["train_metrics_steps"] = m["steps"]

    # ---- eval_step (captured after one eager call)
    tr = trainers[True]
    for _ in range(3):
        tr.eval_step(pc, labels, smpw)
    assert tr._eval_graph is not None
    ev = [region_ms(lambda: tr.eval_step(pc, labels, smpw, sync=False), 20) for _ in range(5)]
    out["eval_step_ms_b16"] = round(float(np.median(ev)), 4)
    out["eval_regions"] = [round(v, 4) for v in ev]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
