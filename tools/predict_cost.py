"""What whole-scene prediction costs: one JSON line, measurements and no thresholds.
  * per synthetic scene (a raw cloud as the dense side, its down_sample_arrays result as the store; the shapes of
    semantic.json: N = 8192, batches of 64) the milliseconds of each stage of pn2.predict.predict_scene + label_dense, each
    stage timed on its own over the same batches with a host clock around a device synchronise: sampling
    (sample_batch_in_file), forward (Predictor.predict, replays only), collection (the float32 / int32 copies into the
    collectors), counting (the sparse increment_from_list), interpolation (interpolate_label_with_color over the dense cloud)
    and the dense counting;
  * pn2_label_confusion against the torch lines it replaces in ConfusionMatrix.increment_from_list (kept here for the
    comparison), int32 labels, C = 9, at 2^20 and 10^8 pairs: median of five regions each (a region is a run of back-to-back
    calls between two synchronisations: 128 calls at 2^20 pairs, one at 10^8), the two alternating in one run, and the
    allocator's peak across one call of each.
usage: python tools/predict_cost.py [--scene-points 4000000] [--num-samples 128] [--pairs 1048576,100000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402

M = pn2.util.metric


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def synthetic_scene(seed, n, ex, ey):
    rs = np.random.RandomState(seed)
    xy = np.stack([rs.uniform(0, ex, n), rs.uniform(0, ey, n)], 1)
    z = np.abs(rs.normal(0, 1.0, n)) + 4.0 * ((xy[:, 0] // 10 + xy[:, 1] // 10) % 3 == 0) * rs.uniform(0, 1, n)
    points = np.concatenate([xy, z[:, None]], 1).astype(np.float32).astype(np.float64)
    labels = np.clip((z / 0.7).astype(np.int32) + 1, 1, 8)
    colors = np.clip(np.stack([z / 5.0, xy[:, 0] / ex, xy[:, 1] / ey], 1) + rs.normal(0, 0.05, (n, 3)), 0, 1)
    return points, labels, colors


def torch_increment(counts, c, gt_labels, pd_labels):
    """the device branch of ConfusionMatrix.increment_from_list before pn2_label_confusion"""
    gt = gt_labels.reshape(-1).long()
    pd = pd_labels.reshape(-1).long()
    ok = (gt >= 0) & (gt < c) & (pd >= 0) & (pd < c)
    idx = torch.where(ok, gt * c + pd, torch.full_like(gt, c * c + 1))
    counts.scatter_add_(0, idx, torch.ones_like(idx))
    counts[c * c + 1:].zero_()


def scene_stages(args, dev, out):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    N, B = hp["num_point"], 64
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    scenes, dense = [], []
    for k, (ex, ey) in enumerate(((60.0, 40.0), (40.0, 30.0))):
        pts, labels, colors = synthetic_scene(200 + k, args.scene_points, ex, ey)
        sp, sc, sl = pn2.downsample.down_sample_arrays(t(pts, torch.float64), t(colors, torch.float64), t(labels, torch.int32), 0.05)
        scenes.append((sp.cpu().numpy(), sl.cpu().numpy(), sc.cpu().numpy(), "syn%d" % k))
        dense.append((t(pts, torch.float32), t(labels, torch.int32)))
    ds = pn2.dataset.SemanticDataset(N, "validation", True, 10, 10, "", device=dev, scenes=scenes)
    predictor = pn2.predict.Predictor(None, 9, hp, device=dev)
    sizes = [min(B, args.num_samples - i) for i in range(0, args.num_samples, B)]
    for b in set(sizes):  # warm every shape: store upload, graph capture
        predictor.predict(ds.sample_batch_in_file(0, b)[0])
    out["scenes"] = []
    for k in range(ds.num_scenes):
        rec = {"scene_points_store": int(ds.scene_counts[k]), "dense_points": int(dense[k][0].shape[0]),
               "num_samples": args.num_samples, "batches": sizes}
        rec["sampling_ms"], batches = timed_ms(lambda: [ds.sample_batch_in_file(k, b) for b in sizes])
        rec["forward_ms"], preds = timed_ms(lambda: [predictor.predict(x[0]) for x in batches])
        points = torch.empty((args.num_samples * N, 3), dtype=torch.float32, device=dev)
        labels = torch.empty((args.num_samples * N,), dtype=torch.int32, device=dev)

        def collect():
            at = 0
            for (_, raw, _), p in zip(batches, preds):
                m = p.numel()
                points[at:at + m].copy_(raw.reshape(-1, 3))
                labels[at:at + m].copy_(p.reshape(-1))
                at += m
        rec["collection_ms"], _ = timed_ms(collect)
        cm = M.ConfusionMatrix(9, device=dev)
        rec["counting_sparse_ms"], _ = timed_ms(lambda: [cm.increment_from_list(x[2].reshape(-1), p.reshape(-1))
                                                         for x, p in zip(batches, preds)])
        dp, dgt = dense[k]
        pn2.interpolate_label_with_color(points, labels, dp[:1024], 3)  # first use
        rec["interpolation_ms"], (dl, _) = timed_ms(lambda: pn2.predict.label_dense(points, labels, dp))
        cmd = M.ConfusionMatrix(9, device=dev)
        rec["counting_dense_ms"], _ = timed_ms(lambda: cmd.increment_from_list(dgt, dl))
        rec["whole_scene_ms"], _ = timed_ms(lambda: pn2.predict.label_dense(
            *pn2.predict.predict_scene(predictor, ds, k, args.num_samples, B, confusion=cm), dp, dgt, confusion=cmd))
        ds.check_last()
        out["scenes"].append({a: (round(v, 3) if isinstance(v, float) else v) for a, v in rec.items()})


def counting(args, dev, out):
    C = 9
    out["label_confusion"] = []
    for n in [int(v) for v in args.pairs.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(n % 1000)
        gt = torch.randint(-1, C + 1, (n,), generator=gen, device=dev, dtype=torch.int32)
        pd = torch.randint(0, C, (n,), generator=gen, device=dev, dtype=torch.int32)
        a, b = M.ConfusionMatrix(C, device=dev), M.ConfusionMatrix(C, device=dev)
        rec = {"pairs": n}
        for name, fn in (("kernel", lambda: a.increment_from_list(gt, pd)), ("torch", lambda: torch_increment(b.counts, C, gt, pd))):
            fn()  # first use
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            rec[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - before)
        # one region = `calls` back-to-back calls between two synchronisations, so that a small size is not a measurement of
        # one launch and one synchronise: 128 calls at 2^20 pairs, one at 10^8
        calls = int(max(1, min(200, (1 << 27) // n)))
        rec["calls_per_region"] = calls
        ker, tor = [], []
        for _ in range(5):  # alternating
            ker.append(timed_ms(lambda: [a.increment_from_list(gt, pd) for _ in range(calls)])[0] / calls)
            tor.append(timed_ms(lambda: [torch_increment(b.counts, C, gt, pd) for _ in range(calls)])[0] / calls)
        assert torch.equal(a.counts, b.counts)  # the same number of calls each: the same counts
        rec.update(kernel_ms=round(float(np.median(ker)), 4), torch_ms=round(float(np.median(tor)), 4),
                   kernel_calls_ms=[round(v, 4) for v in ker], torch_calls_ms=[round(v, 4) for v in tor],
                   kernel_GBps=round(8.0 * n / (float(np.median(ker)) * 1e-3) * 1e-9, 1))
        out["label_confusion"].append(rec)
        del gt, pd
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene-points", type=int, default=4000000, help="raw points per synthetic scene")
    ap.add_argument("--num-samples", type=int, default=128)
    ap.add_argument("--pairs", default="1048576,100000000")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    counting(args, dev, out)
    scene_stages(args, dev, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
