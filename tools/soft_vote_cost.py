"""What soft voting costs against the hard vote it stands beside ("Soft voting"): one JSON line with, in
this one process, medians of 5 regions, the device synchronised on both sides of each:
  1 scene   predict.predict_scene_tiled on the 1.5 M-point synthetic scene syn_a of examples/train_semantic3d.py (N = 8192,
            B = 64, fresh weights), one grid and two, vote="soft" against vote="hard";
  2 steps   the vote and label launches of a pass alone, on the pass's own batches: pn2_tile_vote_scores + pn2_score_labels
            against pn2_tile_vote + pn2_tile_labels, and pn2_softmax_scores on one (64, 8192, 9) batch of logits; the soft vote
            also in the one-row-per-lane form restated in torch (index_add_ of int64 rows), checked to give the same sums first;
  3 dense   pn2_interpolate_scores against pn2_interpolate_label_with_color at 1 M sparse / 10 M dense points, C = 9, knn = 3,
            one call each over the whole dense cloud; --dense-only / --skip-dense select.
usage: python tools/soft_vote_cost.py [--skip-dense] [--dense-only] [--sparse 1000000] [--dense 10000000]"""
import argparse
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

launch, ptr = pn2._lib.launch, pn2._lib.ptr

N, B, C = 8192, 64, 9
BOX = 10.0
TWO = ((0.0, 0.0), (BOX / 2, BOX / 2))


def wall_ms(fn, reps=5):
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(v)), 3), [round(x, 3) for x in v]


def scene_cost(dev, out):
    scenes = [ex.synthetic_scene(*ex.SYNTHETIC["syn_a"]) + ("syn_a",)]
    ds = pn2.dataset.SemanticDataset(N, "train", True, BOX, BOX, "", device=dev, seed=0, scenes=scenes, ingest="device")
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(num_point=N, use_color=1)
    predictor = pn2.predict.Predictor(None, C, hp, device=dev)
    tiled = pn2.predict.predict_scene_tiled
    n = int(ds.scene_counts[0])
    out["scene"] = o = {"points": n}
    for vote in ("hard", "soft"):  # the captures
        tiled(predictor, ds, 0, B, vote=vote)
    for name, phases in (("1_grid", TWO[:1]), ("2_grids", TWO)):
        for vote in ("hard", "soft"):
            o["%s_%s_ms" % (name, vote)], o["%s_%s_runs" % (name, vote)] = wall_ms(lambda: tiled(predictor, ds, 0, B, phases=phases, vote=vote))
    o["graphs"] = [len(predictor._graphs), len(predictor._score_graphs)]
    lh, _ = tiled(predictor, ds, 0, B, phases=TWO)
    ls, sc = tiled(predictor, ds, 0, B, phases=TWO, vote="soft")
    o["labels_that_differ_2_grids"] = int((lh != ls).sum())  # fresh weights: how often the two rules part, not an accuracy

    # the steps alone, on the batches of one pass
    st = out["steps"] = {}
    cover = ds.tile_cover(0, (0.0, 0.0), 1)
    batches = []
    for q0 in range(0, cover.num_samples, B):
        data, sel, live = cover.batch(q0, B)
        pred, q = predictor.predict_labels_and_scores(data)
        batches.append((sel.clone(), live.clone(), pred, q))
    st["batches"] = len(batches)
    votes = torch.zeros((n, C), dtype=torch.int32, device=dev)
    scores = torch.zeros((n, C), dtype=torch.int64, device=dev)
    t_scores = torch.zeros((n, C), dtype=torch.int64, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    conf = torch.empty((n,), dtype=torch.float32, device=dev)

    def hard_vote():
        for s_, l_, p_, _ in batches:
            launch("pn2_tile_vote", dev, B, N, C, ptr(s_), ptr(l_), ptr(p_), ptr(votes), None)

    def soft_vote():
        for s_, l_, _, q_ in batches:
            launch("pn2_tile_vote_scores", dev, B, N, C, ptr(s_), ptr(l_), ptr(q_), ptr(scores), None)

    def torch_soft_vote():  # whole rows: one row per index, num_class strided adds behind it
        k = torch.arange(N, device=dev)[None, :]
        for s_, l_, _, q_ in batches:
            ok = k < l_[:, None]
            t_scores.index_add_(0, s_[ok].long(), q_[ok].long())
    soft_vote()
    torch_soft_vote()
    assert torch.equal(scores, t_scores), "the torch restatement disagrees (soft vote)"
    st["vote_hard_ms"], st["vote_hard_runs"] = wall_ms(hard_vote)
    st["vote_soft_ms"], st["vote_soft_runs"] = wall_ms(soft_vote)
    st["vote_soft_torch_ms"], st["vote_soft_torch_runs"] = wall_ms(torch_soft_vote)
    st["labels_hard_ms"], st["labels_hard_runs"] = wall_ms(lambda: launch("pn2_tile_labels", dev, n, C, ptr(votes), ptr(labels)))
    st["labels_soft_ms"], st["labels_soft_runs"] = wall_ms(lambda: launch("pn2_score_labels", dev, n, C, ptr(scores), ptr(labels), None))
    st["labels_soft_confidence_ms"], st["labels_soft_confidence_runs"] = wall_ms(
        lambda: launch("pn2_score_labels", dev, n, C, ptr(scores), ptr(labels), ptr(conf)))
    logits = torch.randn((B * N, C), dtype=torch.float32, device=dev) * 3
    q = torch.empty((B * N, C), dtype=torch.int32, device=dev)
    st["softmax_ms"], st["softmax_runs"] = wall_ms(lambda: launch("pn2_softmax_scores", dev, B * N, C, ptr(logits), ptr(q), None))


def dense_cost(dev, out, ns, nd):
    rs = np.random.RandomState(0)
    # a 100 m x 100 m x 10 m slab, the sparse side a sample of the same surface as the dense side
    sp = torch.from_numpy((rs.random_sample((ns, 3)) * [100.0, 100.0, 10.0]).astype(np.float32)).to(dev)
    dp = torch.from_numpy((rs.random_sample((nd, 3)) * [100.0, 100.0, 10.0]).astype(np.float32)).to(dev)
    sc = torch.from_numpy(rs.randint(0, 1 << 31, (ns, C), dtype=np.int64)).to(dev)
    sl = sc.argmax(1).int()
    hard = lambda: pn2.interpolate_label_with_color(sp, sl, dp, 3)  # noqa: E731
    soft = lambda: pn2.tf_ops.tf_interpolate.interpolate_scores_with_color(sp, sc, dp, 3)  # noqa: E731
    hard(), soft()  # first use: the sort's, the allocator's
    d = out["dense"] = {"sparse": ns, "dense": nd, "num_class": C, "knn": 3}
    d["label_ms"], d["label_runs"] = wall_ms(hard)
    d["scores_ms"], d["scores_runs"] = wall_ms(soft)
    d["score_row_bytes_per_dense_point"] = 3 * C * 8
    # the part both share (grid build + search) with a tail that reads next to nothing: one class
    one = sc[:, :1].contiguous()
    d["scores_1_class_ms"], d["scores_1_class_runs"] = wall_ms(
        lambda: pn2.tf_ops.tf_interpolate.interpolate_scores_with_color(sp, one, dp, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--sparse", type=int, default=1000000)
    ap.add_argument("--dense", type=int, default=10000000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"N": N, "B": B, "num_class": C}
    if not args.dense_only:
        scene_cost(dev, out)
    if not args.skip_dense:
        dense_cost(dev, out, args.sparse, args.dense)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
