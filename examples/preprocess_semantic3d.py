#!/usr/bin/env python
"""The reference's preprocess.py followed by its downsample.py, on the device and without the files in between:

    per scene:  <raw>/<scene>.txt (`x y z intensity r g b` per line) and, where it exists, <raw>/<scene>.labels
                -> parsed on the device (pn2.read_semantic3d_txt / pn2.load_labels)
                -> pn2.downsample.down_sample_arrays (label 0 skipped, voxel grid, majority label)
                -> <out>/<scene>.pcd and <out>/<scene>.labels, what SemanticDataset and examples/predict_semantic3d.py read

    --raw PATH          the raw directory (dataset/semantic_raw); every <scene>.txt in it is processed.  Without it a small
                        synthetic raw directory is written first (--scenes K scenes of --points N lines)
    --out PATH          the down-sampled directory (dataset/semantic_downsampled); default <raw>/../semantic_downsampled
    --voxel V           voxel size, 0.05 as in the reference
    --write-dense-pcd   also keep the intermediate <raw>/<scene>.pcd the reference writes (pn2.point_cloud_txt_to_pcd)

A scene whose outputs exist is skipped, as the reference does.

usage: python examples/preprocess_semantic3d.py [--raw PATH] [--out PATH] [--voxel 0.05] [--write-dense-pcd]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pn2_amd as pn2  # noqa: E402

U = pn2.util.point_cloud_util


def write_synthetic_raw(raw_dir, scenes, points):
    """ground + blocks of "buildings" as raw Semantic3D text: millimetre coordinates, an intensity that is now and then a
    non-integer (the reason preprocess.py:44 exists), 8-bit colours; every other scene has labels (0 = unlabeled .. 8)"""
    for k in range(scenes):
        rs = np.random.RandomState(100 + k)
        ex, ey = 30.0 + 10.0 * (k % 2), 20.0 + 10.0 * (k % 3)
        xy = np.stack([rs.uniform(0, ex, points), rs.uniform(0, ey, points)], 1)
        z = np.abs(rs.normal(0, 1.0, points)) + 4.0 * ((xy[:, 0] // 10 + xy[:, 1] // 10) % 3 == 0) * rs.uniform(0, 1, points)
        inten = rs.randint(-2047, 2048, points)
        rgb = np.clip(np.stack([z / 5.0, xy[:, 0] / ex, xy[:, 1] / ey], 1) * 255.0, 0, 255).astype(np.int64)
        with open(os.path.join(raw_dir, "syn_%d.txt" % k), "w") as f:
            for i, ((x, y), zz, it, (r, g, b)) in enumerate(zip(xy.tolist(), z.tolist(), inten.tolist(), rgb.tolist())):
                f.write("%.3f %.3f %.3f %s %d %d %d\n" % (x, y, zz, it if i % 50 else "%.1f" % (it + 0.5), r, g, b))
        if k % 2 == 0:
            labels = np.where(rs.uniform(0, 1, points) < 0.1, 0, np.clip((z / 0.7).astype(np.int64) + 1, 1, 8))
            U.write_labels(os.path.join(raw_dir, "syn_%d.labels" % k), labels)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw")
    ap.add_argument("--out")
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--write-dense-pcd", action="store_true")
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--points", type=int, default=200000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    raw_dir = args.raw
    if raw_dir is None:
        raw_dir = os.path.join(tempfile.mkdtemp(prefix="semantic_"), "semantic_raw")
        os.makedirs(raw_dir)
        write_synthetic_raw(raw_dir, args.scenes, args.points)
        print("synthetic raw directory: %s" % raw_dir)
    out_dir = args.out or os.path.join(os.path.dirname(os.path.abspath(raw_dir)), "semantic_downsampled")
    os.makedirs(out_dir, exist_ok=True)

    for name in sorted(f[:-4] for f in os.listdir(raw_dir) if f.endswith(".txt")):
        txt, dense_labels = os.path.join(raw_dir, name + ".txt"), os.path.join(raw_dir, name + ".labels")
        sparse_pcd, sparse_labels = os.path.join(out_dir, name + ".pcd"), os.path.join(out_dir, name + ".labels")
        if os.path.isfile(sparse_pcd) and (not os.path.isfile(dense_labels) or os.path.isfile(sparse_labels)):
            print("Skipped:", name)
            continue
        print("Processing:", name)
        t0 = time.time()
        points, colors, _ = pn2.read_semantic3d_txt(txt, dev)
        labels = pn2.load_labels(dense_labels, dev) if os.path.isfile(dense_labels) else None
        if labels is not None and labels.numel() != points.shape[0]:
            raise ValueError("%s: %d points but %d labels" % (name, points.shape[0], labels.numel()))
        torch.cuda.synchronize()
        t1 = time.time()
        print("Num points: %d  (%.1f MB of text parsed in %.2f s)" % (points.shape[0], os.path.getsize(txt) / 1e6, t1 - t0))
        if args.write_dense_pcd:
            pn2.point_cloud_txt_to_pcd(raw_dir, name, dev)
        sp, sc, sl = pn2.downsample.down_sample_arrays(points, colors, labels, voxel_size=args.voxel)
        print("Num points after down sampling:", sp.shape[0])
        pn2.write_point_cloud_pcd(sparse_pcd, sp, sc)
        print("Point cloud written to:", sparse_pcd)
        if sl is not None:
            pn2.write_labels(sparse_labels, sl)
            print("Labels written to:", sparse_labels)
    return 0


if __name__ == "__main__":
    sys.exit(main())
