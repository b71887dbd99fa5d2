"""What the device-side augmentation costs ("Augmentation"): one JSON line with
  (a) one fused util.provider.Augmenter call with every stage on (shuffle, rotation + perturbation, scale, shift, jitter,
      dropout) on a resident batch, B=16, N=8192, C=6, eager calls back to back and as a replayed one-call graph;
  (b) SemanticDataset.sample_batch_in_all_files with its own rotation against the same call with that Augmenter, on the
      synthetic store of examples/train_semantic3d.py, region by region in the same run;
  (c) the captured training step fed through the prefetch path (next batch sampled on a side stream), Augmenter on and off,
      region by region in the same run -- and with an Augmenter that only rotates about z, which hands the step the same
      kind of batch as the sampler's own rotation: the step's time depends on its data (dropout and scale change how many
      ball-query rows are live), so this third figure is the one that isolates the cost of the extra launches; a fourth
      runs every stage but the dropout, which is the stage that changes the batch most (up to 7/8 of a cloud's rows become
      copies of one point);
  (d) the same stages the reference's way: device -> host, the numpy functions of the reference's util/provider.py (restated
      below from their behaviour), host -> device.
Every figure is the median of 5 regions (20 calls / steps each).  usage: python tools/augment_cost.py"""
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

STAGES = dict(rotate="z", perturb=(0.06, 0.18), scale=(0.8, 1.25), shift=0.1, jitter=(0.01, 0.05), dropout=0.875, shuffle=True)


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


def host_way(data, labels, weights):
    """device -> host, numpy in the reference's order of operations, host -> device"""
    x, lab, w = data.cpu().numpy(), labels.cpu().numpy(), weights.cpu().numpy()
    b, n, _ = x.shape
    idx = np.arange(n)
    np.random.shuffle(idx)
    x, lab, w = x[:, idx, :], lab[:, idx], w[:, idx]
    out = np.zeros(x.shape, dtype=np.float32)
    out[:, :, 3:] = x[:, :, 3:]
    for k in range(b):
        a = np.random.uniform() * 2 * np.pi
        r = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]])
        g = np.clip(0.06 * np.random.randn(3), -0.18, 0.18)
        rx = np.array([[1, 0, 0], [0, np.cos(g[0]), -np.sin(g[0])], [0, np.sin(g[0]), np.cos(g[0])]])
        ry = np.array([[np.cos(g[1]), 0, np.sin(g[1])], [0, 1, 0], [-np.sin(g[1]), 0, np.cos(g[1])]])
        rz = np.array([[np.cos(g[2]), -np.sin(g[2]), 0], [np.sin(g[2]), np.cos(g[2]), 0], [0, 0, 1]])
        out[k, :, 0:3] = np.dot(x[k, :, 0:3], np.dot(r, np.dot(rz, np.dot(ry, rx))))
    xyz = out[:, :, 0:3]
    xyz *= np.random.uniform(0.8, 1.25, b)[:, None, None]
    xyz += np.random.uniform(-0.1, 0.1, (b, 3))[:, None, :]
    xyz += np.clip(0.01 * np.random.randn(b, n, 3), -0.05, 0.05)
    for k in range(b):
        drop = np.where(np.random.random(n) <= np.random.random() * 0.875)[0]
        if len(drop) > 0:
            out[k, drop, :] = out[k, 0, :]
    dev = data.device
    return torch.from_numpy(out).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(w).to(dev)


def main():
    dev = torch.device("cuda:0")
    B, N = 16, 8192
    out = {"B": B, "N": N, "C": 6, "stages": sorted(STAGES)}
    scenes = {k: ex.synthetic_scene(*v) + (k,) for k, v in ex.SYNTHETIC.items()}
    train = [scenes[k] for k in ex.SYNTHETIC_SPLITS["train"]]
    ds = pn2.dataset.SemanticDataset(N, "train", True, 10, 10, "", device=dev, seed=0, scenes=train)
    aug = pn2.util.provider.Augmenter(seed=0, device=dev, **STAGES)
    batch = ds.sample_batch_in_all_files(B, augment=False)

    # ---- (a) one fused call on a resident batch
    aug(*batch)
    out["a_call_ms"], out["a_regions"] = med(lambda: aug(*batch))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            aug(*batch)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    out["a_graph_replay_ms"], _ = med(g.replay)
    out["a_launches_per_call"] = 3  # prologue, permutation, rows (csrc/pn2_augment.hip)
    no_shuffle = pn2.util.provider.Augmenter(seed=0, device=dev, **dict(STAGES, shuffle=False))
    no_shuffle(*batch)
    out["a_call_without_shuffle_ms"], _ = med(lambda: no_shuffle(*batch))  # two launches: what the permutation costs

    # ---- (b) the sampler alone and with the Augmenter, alternating regions
    plain, with_aug = [], []
    ds.sample_batch_in_all_files(B, augment=aug)
    for _ in range(5):
        plain.append(region_ms(lambda: ds.sample_batch_in_all_files(B, augment=True)))
        with_aug.append(region_ms(lambda: ds.sample_batch_in_all_files(B, augment=aug)))
    out["b_sampler_ms"], out["b_sampler_augmenter_ms"] = round(float(np.median(plain)), 4), round(float(np.median(with_aug)), 4)
    out["b_regions_sampler"], out["b_regions_sampler_augmenter"] = [round(v, 4) for v in plain], [round(v, 4) for v in with_aug]
    ds.check_last()

    # ---- (d) the host round trip (before the trainers take their memory; numpy on whatever CPU this process has)
    host_way(*batch)
    out["d_host_round_trip_ms"], out["d_regions"] = med(lambda: host_way(*batch), k=5)

    # ---- (c) the captured training step through the prefetch path, Augmenter on and off
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    side = torch.cuda.Stream()
    steps = {}
    rotate_only = pn2.util.provider.Augmenter(seed=0, device=dev, rotate="z")
    no_dropout = pn2.util.provider.Augmenter(seed=0, device=dev, **{k: v for k, v in STAGES.items() if k != "dropout"})
    for name, how in (("off", True), ("on", aug), ("rotate_only", rotate_only), ("no_dropout", no_dropout)):
        tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev)
        cur = [ds.sample_batch_in_all_files(B, augment=how)]

        def step(tr=tr, cur=cur, how=how):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                nxt = ds.sample_batch_in_all_files(B, augment=how)
            torch.cuda.current_stream().wait_stream(side)
            for t in nxt:
                t.record_stream(torch.cuda.current_stream())
            tr.train_step(*cur[0], sync=False, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2])
            cur[0] = nxt
        for _ in range(7):
            step()
        steps[name] = step
    regions = {name: [] for name in steps}
    for _ in range(5):
        for name in steps:
            regions[name].append(region_ms(steps[name]))
    for name, v in regions.items():
        out["c_step_ms_augmenter_" + name] = round(float(np.median(v)), 4)
        out["c_regions_" + name] = [round(x, 4) for x in v]
    ds.check_last()
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
