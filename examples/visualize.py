"""Look at a scene without a window: the reference's visualize.py, rendered to a PNG on one MI355X.

    python examples/visualize.py --pcd_path P [--labels_path L] [--compare GT.labels] --out IMG.png
                                 [--view top|front|side|iso] [--width 1920 --height 1080] [--size 2] [--perspective]

Without labels the cloud is drawn in the file's own colours; with --labels_path in the label colours of the reference's table;
with --compare as well, the points whose label differs from GT.labels are red and the rest keep their label colour.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

MISMATCH = (255, 0, 0)


def point_colors(flags, device="cuda"):
    """-> points (n,3) float64, colors (n,3) uint8 on the device"""
    if not os.path.isfile(flags.pcd_path):
        raise ValueError("pcd path not found at {}".format(flags.pcd_path))
    points, colors = pn2.read_point_cloud(flags.pcd_path, device, want_colors=not flags.labels_path)
    if not flags.labels_path:
        if flags.compare:
            raise ValueError("--compare needs --labels_path")
        return points, torch.floor(colors * 255.0).to(torch.uint8)  # the byte the file held
    if not os.path.isfile(flags.labels_path):
        raise ValueError("labels path not found at {}".format(flags.labels_path))
    labels = pn2.load_labels(flags.labels_path, device)
    if len(labels) != len(points):
        raise ValueError("len(point_cloud.points) != len(labels)")
    colors = pn2.render.colorize_point_cloud(labels)
    if flags.compare:
        truth = pn2.load_labels(flags.compare, device)
        if len(truth) != len(points):
            raise ValueError("len(point_cloud.points) != len(compare labels)")
        colors[labels != truth] = torch.tensor(MISMATCH, dtype=torch.uint8, device=colors.device)
    return points, colors


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--pcd_path", default="", type=str, required=True)
    parser.add_argument("--labels_path", default="", type=str)
    parser.add_argument("--compare", default="", type=str, help="ground-truth .labels: mismatching points are drawn red")
    parser.add_argument("--out", required=True, help="the image: .png, or .ppm")
    parser.add_argument("--view", default="top", choices=pn2.render.VIEWS)
    parser.add_argument("--width", type=int, default=1920)
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--size", type=int, default=2, help="pixels per point side")
    parser.add_argument("--perspective", action="store_true")
    flags = parser.parse_args()
    points, colors = point_colors(flags)
    image = pn2.render.render_colors(points, colors, flags.view, flags.width, flags.height, flags.size,
                                     perspective=flags.perspective)
    (pn2.render.write_ppm if flags.out.lower().endswith(".ppm") else pn2.render.write_png)(flags.out, image)
    print("{} points -> {}".format(len(points), flags.out))


if __name__ == "__main__":
    main()
