#!/usr/bin/env python
"""The reference's predict.py followed by its interpolate.py, on the device:

    per scene of the split:  num_samples columns predicted in batches of --batch-size (the last one smaller)
                             -> result/sparse/<scene>.pcd and .labels, the sparse confusion matrix
                             the sparse labels voted onto the dense cloud with 3-NN
                             -> result/dense/<scene>.labels and <scene>_colored.pcd, the scene's dense metrics
    at the end:              the sparse metrics and the global dense metrics (print_metrics)

    --ckpt FILE   a checkpoint written by Trainer.save() (without it: fresh random weights, for a dry run)
    --data PATH   the preprocessed (down-sampled) Semantic3D files, <PATH>/<scene>.pcd and .labels (dataset/semantic_data)
    --raw PATH    the dense clouds, <PATH>/<scene>.pcd and, where they exist, .labels (dataset/semantic_raw)
                  (--data and --raw: a scene without a .pcd is read from <scene>.ply where that exists)
    without --data / --raw: small synthetic scenes -- a raw cloud as the dense side, its down_sample_arrays result as the store

    --tiled       instead of num_samples random columns, the tiled cover of the scene (pn2.predict.predict_scene_tiled): every
                  point of the store is predicted --phases times (1: one grid; 2: a second grid shifted by half a box votes
                  too) and the sparse side of the 3-NN vote is the whole store; columns below --min-points points are skipped

    --format      the point-cloud files written under result/: pcd (binary PCD, the default) or ply (binary little-endian PLY,
                  float coordinates, uchar colours)

    --soft        soft voting: the class probabilities (score rows, integers in units of 2^-30) are kept instead of their argmax.
                  With --tiled they are summed over the grids (predict_scene_tiled(vote="soft")), without it they are the score
                  rows of the sampled points (predict_scene(scores=True)); either way the dense cloud takes, per point, the class
                  whose scores summed over its 3 nearest sparse points are the largest (pn2.predict.label_dense_scores)

usage: python examples/predict_semantic3d.py [--ckpt FILE] [--set validation] [--num_samples 8] [--data PATH --raw PATH]
       [--tiled [--phases 1|2] [--min-points K]] [--soft] [--format pcd|ply]
       size flags (synthetic runs, tests): --points N --npoint a,b,c,d --scene-points P --scenes K --voxel V --batch-size B"""
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


def load_scenes(args, hp, dev):
    """-> dataset (the down-sampled store), dense {scene name: (points float32 (nd,3), labels int32 (nd,) or None)}: device
    tensors when read from files (pn2.read_point_cloud / pn2.load_labels), numpy arrays for the synthetic scenes"""
    N = hp["num_point"]
    if args.data:
        ds = pn2.dataset.SemanticDataset(N, args.set, hp["use_color"], hp["box_size_x"], hp["box_size_y"], args.data, device=dev,
                                         ingest=args.ingest)
        dense = {}
        for name in ds.scene_names:
            prefix = os.path.join(args.raw or args.data, name)
            pts, _ = pn2.read_point_cloud(pn2.util.point_cloud_util.scene_path(prefix), dev, want_colors=False)
            labels = pn2.load_labels(prefix + ".labels", dev) if os.path.exists(prefix + ".labels") else None
            dense[name] = (pts.to(torch.float32), labels)
        return ds, dense
    scenes, dense = [], {}
    for k in range(args.scenes):
        name = "syn_%s_%d" % (args.set, k)
        ex, ey = 30.0 + 10.0 * (k % 2), 20.0 + 10.0 * (k % 3)
        pts, labels, colors = synthetic_scene(100 + k, args.scene_points, ex, ey)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
        sp, sc, sl = pn2.downsample.down_sample_arrays(t(pts, torch.float64), t(colors, torch.float64), t(labels, torch.int32),
                                                       voxel_size=args.voxel)
        if args.ingest == "device":  # the down-sampled scene stays where it is
            scenes.append((sp, sl, sc, name))
        else:
            scenes.append((sp.cpu().numpy(), sl.cpu().numpy(), sc.cpu().numpy(), name))
        dense[name] = (pts.astype(np.float32), labels.astype(np.int32))
        print("%s: %d raw points -> %d in the store (voxel %.2f m)" % (name, len(pts), len(scenes[-1][0]), args.voxel))
    ds = pn2.dataset.SemanticDataset(N, args.set, hp["use_color"], hp["box_size_x"], hp["box_size_y"], "", device=dev,
                                     scenes=scenes, ingest=args.ingest)
    return ds, dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_samples", type=int, default=8, help="# samples, each contains num_point points_centered")
    ap.add_argument("--ckpt", default="", help="Checkpoint file (Trainer.save)")
    ap.add_argument("--set", default="validation", help="train, validation, test")
    ap.add_argument("--data", default=None, help="directory of the down-sampled scenes")
    ap.add_argument("--raw", default=None, help="directory of the dense scenes (default: --data)")
    ap.add_argument("--out", default="result", help="output directory")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--points", type=int, default=0, help="points per sample (0: num_point of the hyper-parameters)")
    ap.add_argument("--npoint", default="", help="l1,l2,l3,l4 sample counts (default: the hyper-parameters')")
    ap.add_argument("--scenes", type=int, default=2, help="synthetic scenes")
    ap.add_argument("--scene-points", type=int, default=2000000, help="raw points per synthetic scene")
    ap.add_argument("--voxel", type=float, default=0.1, help="voxel size of the synthetic store")
    ap.add_argument("--chunk", type=int, default=1 << 24, help="dense points per interpolation call")
    ap.add_argument("--ingest", choices=("host", "device"), default="host",
                    help="where the store is sorted and measured: numpy, or pn2_scene_ingest straight into HBM")
    ap.add_argument("--tiled", action="store_true", help="label every point of the store: the tiled cover, not random columns")
    ap.add_argument("--phases", type=int, choices=(1, 2), default=1, help="--tiled: grids that vote (2: one shifted by half a box)")
    ap.add_argument("--min-points", type=int, default=1, help="--tiled: columns with fewer points are skipped")
    ap.add_argument("--format", choices=("pcd", "ply"), default="pcd", help="format of the point-cloud files written")
    ap.add_argument("--soft", action="store_true", help="vote with class probabilities instead of labels, through to the dense cloud")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.setdefault("box_size_x", 10)
    hp.setdefault("box_size_y", 10)
    hp["use_color"] = 1
    if args.points:
        hp["num_point"] = args.points
    if args.npoint:
        for k, v in zip(("l1_npoint", "l2_npoint", "l3_npoint", "l4_npoint"), args.npoint.split(",")):
            hp[k] = int(v)
    sparse_dir, dense_dir = os.path.join(args.out, "sparse"), os.path.join(args.out, "dense")
    os.makedirs(sparse_dir, exist_ok=True)
    os.makedirs(dense_dir, exist_ok=True)

    write_cloud = pn2.write_point_cloud_ply if args.format == "ply" else pn2.write_point_cloud_pcd
    dataset, dense = load_scenes(args, hp, dev)
    predictor = pn2.predict.Predictor(args.ckpt or None, dataset.num_classes, hp, device=dev)
    print("Model restored" if args.ckpt else "No checkpoint: random weights")
    cm_sparse = M.ConfusionMatrix(dataset.num_classes, device=dev)
    cm_global = M.ConfusionMatrix(dataset.num_classes, device=dev)
    for k, name in enumerate(dataset.scene_names):
        print("Processing %s" % name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.tiled:
            phases = [(0.0, 0.0), (hp["box_size_x"] / 2, hp["box_size_y"] / 2)][:args.phases]
            labels, scores = pn2.predict.predict_scene_tiled(predictor, dataset, k, args.batch_size, phases, args.min_points,
                                                             confusion=cm_sparse, vote="soft" if args.soft else "hard")
            points = torch.as_tensor(dataset.scene_points[k]).to(dev, torch.float32)  # the whole store is the sparse side
            torch.cuda.synchronize()
            print("    %d points, %d grid(s) of columns in %.1f ms" % (len(points), len(phases), (time.perf_counter() - t0) * 1e3))
        else:
            if args.soft:
                points, labels, scores = pn2.predict.predict_scene(predictor, dataset, k, args.num_samples, args.batch_size,
                                                                   confusion=cm_sparse, scores=True)
            else:
                points, labels = pn2.predict.predict_scene(predictor, dataset, k, args.num_samples, args.batch_size, confusion=cm_sparse)
            dataset.check_last()
            torch.cuda.synchronize()
            print("    %d samples of %d points in %.1f ms" % (args.num_samples, hp["num_point"], (time.perf_counter() - t0) * 1e3))
        write_cloud(os.path.join(sparse_dir, name + "." + args.format), points)
        pn2.write_labels(os.path.join(sparse_dir, name + ".labels"), labels)
        print("    Exported sparse %s and labels to %s" % (args.format, os.path.join(sparse_dir, name)))

        dense_points, dense_gt = dense[name]
        cm = M.ConfusionMatrix(dataset.num_classes, device=dev)
        t0 = time.perf_counter()
        if args.soft:
            dense_labels, dense_colors, confidence = pn2.predict.label_dense_scores(points, scores, dense_points, dense_gt,
                                                                                    confusion=cm, chunk=args.chunk)
        else:
            dense_labels, dense_colors = pn2.predict.label_dense(points, labels, dense_points, dense_gt, confusion=cm, chunk=args.chunk)
        torch.cuda.synchronize()
        print("    KNN interpolation of %d dense points: %.1f ms" % (len(dense_points), (time.perf_counter() - t0) * 1e3))
        if args.soft:
            print("    Soft vote: mean confidence of the dense labels %.4f" % float(confidence.mean()))
        pn2.write_labels(os.path.join(dense_dir, name + ".labels"), dense_labels)
        write_cloud(os.path.join(dense_dir, name + "_colored." + args.format), dense_points, dense_colors)  # uint8 as it is
        print("    Dense labels and coloured %s written to %s" % (args.format, os.path.join(dense_dir, name)))
        if dense_gt is not None:
            cm.print_metrics(dataset.labels_names)
            cm_global.counts += cm.counts
    print("Sparse results")
    cm_sparse.print_metrics(dataset.labels_names)
    print("Global results")
    cm_global.print_metrics(dataset.labels_names)


if __name__ == "__main__":
    main()
