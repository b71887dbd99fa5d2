"""Colour a labelled scene on one MI355X: the reference's colorize.py.

    python examples/colorize.py <in.pcd|.ply> <in.labels> <out.pcd|.ply>
    python examples/colorize.py --pd_dir result/sparse [--gt_dir result/sparse] [--out_dir result/sparse_colorized]

The second form is the reference's __main__: every <pd_dir>/<scene>.labels colours <gt_dir>/<scene>.pcd into
<out_dir>/<scene>.pcd.  The cloud and the labels are read on the device (pn2.read_point_cloud, pn2.load_labels), each label
becomes its colour of the reference's table (pn2.render.colorize_point_cloud), and the device writers take the uint8 colours as
they are: the file carries the table's bytes.
"""
import argparse
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402


def colorize(input_pcd_path, input_labels_path, output_pcd_path):
    points, _ = pn2.read_point_cloud(input_pcd_path, want_colors=False)
    print("Point cloud loaded from", input_pcd_path)
    labels = pn2.load_labels(input_labels_path)
    print("Labels loaded from", input_labels_path)
    if len(points) != len(labels):
        raise ValueError("len(point_cloud.points) != len(labels)")

    s = time.time()
    colors = pn2.render.colorize_point_cloud(labels)
    torch.cuda.synchronize()
    print("time colorize_point_cloud pd", time.time() - s, flush=True)

    ext = os.path.splitext(output_pcd_path)[1].lower()
    if ext == ".pcd":
        pn2.write_point_cloud_pcd(output_pcd_path, points, colors)
    elif ext == ".ply":
        pn2.write_point_cloud_ply(output_pcd_path, points, colors, coord="double")
    else:
        raise ValueError("a scene file is .pcd or .ply, got %s" % output_pcd_path)
    print("Output written to", output_pcd_path)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("paths", nargs="*", help="<in.pcd|.ply> <in.labels> <out.pcd|.ply>")
    parser.add_argument("--pd_dir", default="", help="folder of predicted <scene>.labels")
    parser.add_argument("--gt_dir", default="", help="folder of the <scene>.pcd (default: --pd_dir)")
    parser.add_argument("--out_dir", default="", help="default: <pd_dir>_colorized")
    flags = parser.parse_args()
    if len(flags.paths) == 3 and not flags.pd_dir:
        return colorize(*flags.paths)
    if flags.paths or not flags.pd_dir:
        parser.error("three paths, or --pd_dir")
    gt_dir = flags.gt_dir or flags.pd_dir
    out_dir = flags.out_dir or flags.pd_dir.rstrip("/\\") + "_colorized"
    os.makedirs(out_dir, exist_ok=True)
    for pd_labels_path in sorted(glob.glob(os.path.join(flags.pd_dir, "*.labels"))):
        print("Processing", pd_labels_path)
        file_prefix = os.path.basename(os.path.splitext(pd_labels_path)[0])
        colorize(os.path.join(gt_dir, file_prefix + ".pcd"), pd_labels_path, os.path.join(out_dir, file_prefix + ".pcd"))


if __name__ == "__main__":
    main()
