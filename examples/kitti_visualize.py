"""The frames of a KITTI raw drive as one PNG each: the reference's kitti_visualize.py without its window.

    python examples/kitti_visualize.py --kitti_root <dir> --out DIR [--view top] [--width 1920 --height 1080] [--size 1]
    python examples/kitti_visualize.py --synthetic 3 120000 --out DIR      # no dataset: F frames of N points in the KITTI layout

One Renderer is reused by every frame (clear, splat, image: no allocation per frame).  The view is fitted to the first frame and
kept, as the reference resets its view point once; a point is drawn in the grey of its intensity.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import pn2_amd as pn2  # noqa: E402
from predict_kitti import DATE, write_synthetic_drive  # noqa: E402

DRIVE = "0001"  # kitti_visualize.py:16
GREYS = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)  # a 256-entry palette: "label" g is the grey (g, g, g)


def run(flags, kitti_root, drive):
    os.makedirs(flags.out, exist_ok=True)
    dataset = pn2.dataset.KittiDataset(8192, kitti_root, [DATE], [drive], 10.0, 10.0)
    renderer = pn2.render.Renderer(flags.width, flags.height, flags.size)
    view = None
    for k in range(len(dataset.frames)):
        frame = dataset.read_frame(k)  # (n,4) float32: x, y, z, intensity
        points = frame[:, :3].contiguous()
        if view is None:
            view = pn2.render.fit_view(points, flags.view, flags.width, flags.height)
        grey = (64.0 + 191.0 * frame[:, 3].clamp(0.0, 1.0)).to(torch.int32)  # intensity 0 is still visible on black
        colors = pn2.render.colorize_point_cloud(grey, GREYS)
        renderer.clear()
        renderer.splat(points, view)
        path = os.path.join(flags.out, "%010d.png" % k)
        pn2.render.write_png(path, renderer.image(colors))
        print("frame {}: {} points, {} outside the view -> {}".format(k, len(points), renderer.culled, path))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--kitti_root", default="", help="KITTI raw root; with --synthetic: where the frames are written")
    parser.add_argument("--synthetic", type=int, nargs=2, metavar=("F", "N"), help="write F frames of N points and draw them")
    parser.add_argument("--out", required=True, help="folder of the PNGs")
    parser.add_argument("--view", default="top", choices=pn2.render.VIEWS)
    parser.add_argument("--width", type=int, default=1920)
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--size", type=int, default=1)
    flags = parser.parse_args()
    if not flags.synthetic:
        if not flags.kitti_root:
            parser.error("--kitti_root or --synthetic is required")
        return run(flags, flags.kitti_root, DRIVE)
    from predict_kitti import DRIVE as synthetic_drive  # the drive write_synthetic_drive fills
    if flags.kitti_root:
        write_synthetic_drive(flags.kitti_root, *flags.synthetic)
        return run(flags, flags.kitti_root, synthetic_drive)
    with tempfile.TemporaryDirectory() as root:
        write_synthetic_drive(root, *flags.synthetic)
        run(flags, root, synthetic_drive)


if __name__ == "__main__":
    main()
