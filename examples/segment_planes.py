"""Find the large planes of a scene on one MI355X: floor, road, facades.

    python examples/segment_planes.py --points scene.pcd --threshold 0.05 --max_planes 4 --min_inliers 1000 --out result
    python examples/segment_planes.py --synthetic 6000 --out result

The cloud is read on the device (pn2.read_point_cloud) and pn2.segment_planes peels up to --max_planes planes off it: each is
the best of --trials RANSAC hypotheses over the points that no earlier plane took, and the peeling stops at the first plane with
fewer than --min_inliers points.  The result is written to
    <out>/planes.txt   one line per plane: index count a b c d -- the exact, unnormalised plane a*x + b*y + c*z + d = 0
                       (repr-exact floats)
    <out>/planes.png   the scene from a corner above it, every plane in a colour of its own, everything else grey (pn2.render)
with one line per plane (count, unit normal, offset) on the terminal.  --synthetic N makes a floor, two walls and clutter
(synthetic(N) below).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

SYNTHETIC_THRESHOLD = 0.05


def synthetic(n, seed=0):
    """-> points (n,3) float32: a floor z = 0 (n/2 points), a wall x = 0 (n/3), a wall y = 0 (n/8), each with noise of sigma 0.01
    across it, inside a room of 10 x 10 x 4, and clutter anywhere in the room (the rest); the rows are shuffled."""
    rs = np.random.RandomState(seed)
    sizes = [n // 2, n // 3, n // 8]
    room = rs.uniform(0, 1, (n, 3)) * [10.0, 10.0, 4.0]
    start = 0
    for axis, size in zip((2, 0, 1), sizes):
        room[start:start + size, axis] = rs.normal(0, 0.01, size)
        start += size
    return room[rs.permutation(n)].astype(np.float32)


def plane_ids(planes, n, device):
    """-> (n,) int32: the index of the plane that took each point, -1 for none"""
    ids = torch.full((n,), -1, dtype=torch.int32, device=device)
    for k, plane in enumerate(planes):
        ids[plane.inliers] = k
    return ids


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--points", default="", help="scene.pcd or scene.ply")
    parser.add_argument("--synthetic", type=int, default=0, help="N points of a floor, two walls and clutter instead of a scene")
    parser.add_argument("--threshold", type=float, default=0.0, help="the largest distance of a point from its plane")
    parser.add_argument("--max_planes", type=int, default=4)
    parser.add_argument("--min_inliers", type=int, default=100)
    parser.add_argument("--trials", type=int, default=1024)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--out", default="result/planes")
    parser.add_argument("--width", type=int, default=1280)
    parser.add_argument("--height", type=int, default=960)
    flags = parser.parse_args()
    if flags.synthetic > 0:
        points = torch.from_numpy(synthetic(flags.synthetic)).cuda()
        threshold = flags.threshold or SYNTHETIC_THRESHOLD
    elif flags.points:
        points, _ = pn2.read_point_cloud(flags.points, want_colors=False)
        threshold = flags.threshold
    else:
        parser.error("--points, or --synthetic N")
    if not threshold > 0:
        parser.error("--threshold")

    planes = pn2.segment_planes(points, threshold, flags.max_planes, flags.min_inliers, trials=flags.trials, seed=flags.seed)
    for k, plane in enumerate(planes):
        a, b, c, d = plane.model.tolist()
        print("plane %d: %d points, normal (%.4f, %.4f, %.4f), offset %.4f" % (k, plane.count, a, b, c, d))
    taken = sum(plane.count for plane in planes)
    print("%d planes, %d of %d points on one" % (len(planes), taken, len(points)))

    os.makedirs(flags.out, exist_ok=True)
    with open(os.path.join(flags.out, "planes.txt"), "w") as f:
        for k, plane in enumerate(planes):
            f.write("%d %d %s\n" % (k, plane.count, " ".join(repr(v) for v in plane.raw.tolist())))
    ids = plane_ids(planes, len(points), points.device)
    image = pn2.render.render_colors(points.float(), pn2.cluster_colors(ids), "iso", flags.width, flags.height, size=2)
    pn2.render.write_png(os.path.join(flags.out, "planes.png"), image)
    print("Output written to", flags.out)


if __name__ == "__main__":
    main()
