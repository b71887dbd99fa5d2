#!/usr/bin/env python
"""The reference's epoch loop with its metrics (train.py:199-331: train_one_epoch / eval_one_epoch) on the device, on two
synthetic scenes -- one to train on, one to validate on:

    per epoch:  reset_metrics -> S captured training steps (argmax + confusion matrix + loss sum inside the step's graph)
                -> train_metrics (the epoch's one synchronisation) -> the reference's log lines
                reset_eval_metrics -> V eval_step batches (captured inference forward + loss + counting) -> eval_metrics

It also prints what the metrics cost per training step (the captured step replayed with and without them).
usage: python examples/train_eval_synthetic.py [epochs] [steps_per_epoch] [val_batches] [scene_points]
                                               [--optimizer {adam,momentum}] [--save PATH] [--resume PATH]
--optimizer: the reference's semantic.json "optimizer" (train.py:380-388).  --save: the trainer's state (variables, moving
averages, optimizer slots, step count) after the last epoch; --resume: load such a file before the first step -- the run then
continues where the saved one stopped (same learning-rate staircase, batch-norm decay, dropout stream)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402

M = pn2.util.metric


def make_scene(seed, n_scene, dev):
    """a 60 m x 40 m scene: ground + a few "buildings"; label = height band 1..8 (learnable from xyz + rgb; no label 0, the
    class the Semantic3D metrics ignore)"""
    rs = np.random.RandomState(seed)
    xy = np.stack([rs.uniform(0, 60, n_scene), rs.uniform(0, 40, n_scene)], 1)
    z = np.abs(rs.normal(0, 1.0, n_scene)) + 4.0 * ((xy[:, 0] // 10 + xy[:, 1] // 10) % 3 == 0) * rs.uniform(0, 1, n_scene)
    points = np.concatenate([xy, z[:, None]], 1).astype(np.float32).astype(np.float64)
    labels = np.clip((z / 0.7).astype(np.int32) + 1, 1, 8)
    colors = np.clip(np.stack([z / 5.0, xy[:, 0] / 60.0, xy[:, 1] / 40.0], 1) + rs.normal(0, 0.05, (n_scene, 3)), 0, 1)
    fd = pn2.dataset.SemanticFileData(points=points, labels=labels, colors=colors, box_size_x=10, box_size_y=10, device=dev)
    counts = np.bincount(labels, minlength=9).astype(np.float32)
    label_weights = torch.from_numpy(1.0 / np.log(1.2 + counts / counts.sum())).float().to(dev)  # semantic_dataset.py:282-290
    return fd, label_weights


def log(title, m):
    print(title)
    for line in M.epoch_log_lines(m["mean_loss"], m["per_class_iou"], m["accuracy"], m["mean_iou"]):
        print("    " + line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("epochs", type=int, nargs="?", default=3)
    ap.add_argument("steps_per_epoch", type=int, nargs="?", default=20)
    ap.add_argument("val_batches", type=int, nargs="?", default=4)
    ap.add_argument("scene_points", type=int, nargs="?", default=1000000)
    ap.add_argument("--optimizer", choices=["adam", "momentum"], default="adam")
    ap.add_argument("--save", metavar="PATH", help="write the trainer's state here after the last epoch")
    ap.add_argument("--resume", metavar="PATH", help="load a saved state before the first step")
    args = ap.parse_args()
    epochs, steps, val_batches, n_scene = args.epochs, args.steps_per_epoch, args.val_batches, args.scene_points
    dev = torch.device("cuda:0")
    train_fd, train_w = make_scene(0, n_scene, dev)
    val_fd, val_w = make_scene(1, n_scene, dev)
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS, optimizer=args.optimizer)
    B, N = hp["batch_size"], hp["num_point"]

    def batch(fd, w):
        c, _, lab, col = fd.sample_batch(B, N, capacity=400000)
        return torch.cat([c, col], dim=2), lab.long(), w[lab.long()]

    # the validation set: fixed batches.  (The reference's validation split has all-zero label weights, so its logged
    # validation loss is 0 under SUM_BY_NONZERO_WEIGHTS; here the training weights are used so that the loss says something.)
    val = [batch(val_fd, val_w) for _ in range(val_batches)]
    tr = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev, track_metrics=True)
    if args.resume:
        tr.load(args.resume)  # applied when the first batch (the validation below) creates the variables
        print("resuming from %s" % args.resume)

    def validate(title):
        tr.reset_eval_metrics()
        for v in val:
            tr.eval_step(*v, sync=False)
        m = tr.eval_metrics()
        log(title, m)
        return m

    init = validate("---- validation at initialisation ----")
    for epoch in range(epochs):
        tr.reset_metrics()
        cur = batch(train_fd, train_w)
        for i in range(steps):
            nxt = batch(train_fd, train_w)
            tr.train_step(*cur, sync=False, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2])
            cur = nxt
        log("---- epoch %03d training ----" % epoch, tr.train_metrics())
        last = validate("---- epoch %03d validation ----" % epoch)
    train_fd.check_last()
    val_fd.check_last()
    if args.save:
        tr.save(args.save)
        print("saved the trainer's state after step %d to %s" % (tr.step_count, args.save))
    print("validation accuracy: %.4f at initialisation -> %.4f after %d steps" % (init["accuracy"], last["accuracy"],
                                                                                  epochs * steps))

    # what the metrics cost: the captured step replayed back to back on the batch resident in its static buffers, with the
    # counting (this trainer) and without (a twin built with track_metrics=False)
    twin = pn2.train.Trainer(hp, 9, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev)
    for _ in range(twin.warmup_eager + 2):
        twin.train_step(*cur)

    def replay_ms(t, k=20):
        with torch.cuda.stream(t._stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                t._graph.replay()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    on, off = [], []
    for _ in range(5):
        on.append(replay_ms(tr))
        off.append(replay_ms(twin))
    on_ms, off_ms = float(np.median(on)), float(np.median(off))
    print("metrics overhead: %.4f ms per step (captured step %.4f ms with, %.4f ms without; median of 5 x 20 replays)"
          % (on_ms - off_ms, on_ms, off_ms))


if __name__ == "__main__":
    main()
