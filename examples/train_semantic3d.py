#!/usr/bin/env python
"""The reference's epoch loop (train.py:199-331) fed by the device-resident multi-scene SemanticDataset:

    per epoch:  get_num_batches(B) training steps on the `train` split (augment=True); every next batch is sampled on a side
                stream and handed to the step through next_pc / next_labels / next_smpw
                -> the reference's training log lines
                a validation pass: eval_step on `validation` batches (augment=False; the reference's validation weights are
                all zero, so its logged validation loss is 0) -> the reference's validation log lines

    --data PATH   the preprocessed Semantic3D files (<PATH>/<scene>.pcd and .labels, the reference's dataset/semantic_data)
    without it    a synthetic multi-scene store: scenes of different sizes, dense enough for columns of 50k+ points

    --ingest device
                  the store is built on the device (SemanticDataset(ingest="device")): same store, same log lines wherever
                  no two points of a scene share an x (the order of such rows is the one thing the two paths may differ in)

    --jitter SIGMA CLIP, --scale LO HI, --shift RANGE, --dropout MAX_RATIO, --shuffle
                  the rest of the reference's util/provider.py on the training batches (util.provider.Augmenter, one fused
                  call behind the sampler on the same side stream; it also takes over the z-rotation).  All off by default.

usage: python examples/train_semantic3d.py [--data PATH] [--epochs E] [--max-steps S] [--val-batches V] [augmentation]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402

M = pn2.util.metric


def synthetic_scene(seed, n, ex, ey):
    """ground + blocks of "buildings"; label = height band 1..8, colour from height and position"""
    rs = np.random.RandomState(seed)
    xy = np.stack([rs.uniform(0, ex, n), rs.uniform(0, ey, n)], 1)
    z = np.abs(rs.normal(0, 1.0, n)) + 4.0 * ((xy[:, 0] // 10 + xy[:, 1] // 10) % 3 == 0) * rs.uniform(0, 1, n)
    points = np.concatenate([xy, z[:, None]], 1).astype(np.float32).astype(np.float64)
    labels = np.clip((z / 0.7).astype(np.int32) + 1, 1, 8)
    colors = np.clip(np.stack([z / 5.0, xy[:, 0] / ex, xy[:, 1] / ey], 1) + rs.normal(0, 0.05, (n, 3)), 0, 1)
    return points, labels, colors


# name -> (seed, points, x extent, y extent): ~600 points per m^2, so a 10 m x 10 m column holds ~60k points
SYNTHETIC = {"syn_a": (0, 1500000, 60.0, 40.0), "syn_b": (1, 800000, 40.0, 30.0), "syn_c": (2, 500000, 30.0, 30.0),
             "syn_d": (3, 700000, 40.0, 30.0), "syn_e": (4, 400000, 30.0, 20.0)}
SYNTHETIC_SPLITS = {"train": ["syn_a", "syn_b", "syn_c"], "validation": ["syn_d", "syn_e"]}


def datasets(args, hp, dev):
    kw = dict(device=dev, ingest=args.ingest)
    N = hp["num_point"]
    if args.data:
        mk = lambda split, seed: pn2.dataset.SemanticDataset(N, split, hp["use_color"], hp["box_size_x"],  # noqa: E731
                                                              hp["box_size_y"], args.data, seed=seed, **kw)
    else:
        scenes = {k: synthetic_scene(*v) + (k,) for k, v in SYNTHETIC.items()}
        mk = lambda split, seed: pn2.dataset.SemanticDataset(  # noqa: E731
            N, split, hp["use_color"], hp["box_size_x"], hp["box_size_y"], "", seed=seed,
            scenes=[scenes[k] for k in SYNTHETIC_SPLITS[split]], **kw)
    return mk("train", 0), mk("validation", 1)


def add_augmentation_arguments(ap):
    ap.add_argument("--jitter", type=float, nargs=2, metavar=("SIGMA", "CLIP"), default=None)
    ap.add_argument("--scale", type=float, nargs=2, metavar=("LO", "HI"), default=None)
    ap.add_argument("--shift", type=float, metavar="RANGE", default=None)
    ap.add_argument("--dropout", type=float, metavar="MAX_RATIO", default=None)
    ap.add_argument("--shuffle", action="store_true")


def augmenter(args, dev, rotate=None, seed=0):
    """the Augmenter the command line asks for, or None when it asks for none (the default run is then unchanged)"""
    if args.jitter is None and args.scale is None and args.shift is None and args.dropout is None and not args.shuffle:
        return None
    return pn2.util.provider.Augmenter(seed=seed, device=dev, rotate=rotate, jitter=args.jitter, scale=args.scale,
                                       shift=args.shift, dropout=args.dropout, shuffle=args.shuffle)


def log(title, m):
    print(title)
    for line in M.epoch_log_lines(m["mean_loss"], m["per_class_iou"], m["accuracy"], m["mean_iou"]):
        print("    " + line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--max-steps", type=int, default=0, help="cap the training steps per epoch (0: get_num_batches)")
    ap.add_argument("--val-batches", type=int, default=0, help="validation batches (0: get_num_batches of validation)")
    ap.add_argument("--ingest", choices=("host", "device"), default="host",
                    help="where the store is sorted and measured: numpy, or pn2_scene_ingest straight into HBM")
    add_augmentation_arguments(ap)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.setdefault("use_color", True)
    hp.setdefault("box_size_x", 10)
    hp.setdefault("box_size_y", 10)
    B = hp["batch_size"]
    train, val = datasets(args, hp, dev)
    print("train: %d scenes, %d points, %d batches per epoch; validation: %d scenes, %d points"
          % (train.num_scenes, train.get_total_num_points(), train.get_num_batches(B), val.num_scenes,
             val.get_total_num_points()))
    tr = pn2.train.Trainer(hp, train.num_classes, store=pn2.util.tf_util.VariableStore(device=dev, seed=0), device=dev,
                           track_metrics=True)
    side = torch.cuda.Stream()
    aug = augmenter(args, dev, rotate="z") or True  # True: the sampler's own z-rotation, as before

    def sample_next(ds, augment):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            nxt = ds.sample_batch_in_all_files(B, augment=augment)
        torch.cuda.current_stream().wait_stream(side)
        for t in nxt:
            t.record_stream(torch.cuda.current_stream())
        return nxt

    for epoch in range(args.epochs):
        print("**** EPOCH %03d ****" % epoch)
        steps = train.get_num_batches(B)
        if args.max_steps:
            steps = min(steps, args.max_steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cur = train.sample_batch_in_all_files(B, augment=aug)
        for _ in range(steps):
            nxt = sample_next(train, aug)
            tr.train_step(*cur, sync=False, next_pc=nxt[0], next_labels=nxt[1], next_smpw=nxt[2])
            cur = nxt
        m = tr.train_metrics()
        dt = time.perf_counter() - t0
        tr.reset_metrics()  # the next epoch counts from zero (the trainer's counters exist after its first step)
        log("---- EPOCH %03d TRAINING ----" % epoch, m)
        print("    %d steps in %.2f s (%.2f ms per step, sampling included)" % (steps, dt, dt / max(1, steps) * 1e3))
        train.check_last()

        nval = args.val_batches or max(1, val.get_num_batches(B))
        tr.reset_eval_metrics()
        for _ in range(nval):
            tr.eval_step(*val.sample_batch_in_all_files(B, augment=False), sync=False)
        log("---- EPOCH %03d EVALUATION ----" % epoch, tr.eval_metrics())
        val.check_last()


if __name__ == "__main__":
    main()
