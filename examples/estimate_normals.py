"""Surface normals and stray points of a scene on one MI355X: which way the surface faces at every point, and which points have
nobody around them.

    python examples/estimate_normals.py scene.pcd --radius 0.3 --nb_points 5 --out result
    python examples/estimate_normals.py --synthetic 3000 --out result

The cloud is read on the device (pn2.read_point_cloud), pn2.radius_neighborhoods counts the points within --radius of every
point and fits a plane to them, and the result is written to
    <out>/normals.png    the scene from above, every point in the colour of its normal (pn2.normal_colors: x, y, z as red, green,
                         blue around mid-grey), points with fewer than --min_neighbors points around them grey (pn2.render)
    <out>/outliers.txt   one line per point with fewer than --nb_points points within the radius, itself counted: its index
                         (what pn2.remove_radius_outlier removes)
with the counts on the terminal.  --viewpoint X Y Z turns every normal to that side (a sensor at the origin: 0 0 0).
--synthetic N makes a wavy sheet of N - N // 50 points and N // 50 points scattered far above it (synthetic(N) below), so the
expected outliers are known."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

SYNTHETIC_RADIUS = 0.5
SYNTHETIC_NB_POINTS = 2


def synthetic(n, seed=0):
    """-> points (n,3) float32, planted (n,) bool: a wavy sheet over [0, s] x [0, s], s chosen for 40 points per unit square (a
    point has about 30 within SYNTHETIC_RADIUS), and n // 50 planted points on a lattice of spacing 2 at height 6 above it, each
    alone within the radius; the rows are shuffled."""
    rs = np.random.RandomState(seed)
    stray = n // 50
    sheet = n - stray
    s = np.sqrt(sheet / 40.0)
    xy = rs.uniform(0, s, (sheet, 2))
    z = 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1])
    k = np.arange(stray)
    side = int(np.ceil(np.sqrt(max(stray, 1))))
    planted = np.stack([(k % side) * 2.0, (k // side) * 2.0, np.full(stray, 6.0)], 1)
    points = np.concatenate([np.concatenate([xy, z[:, None]], 1), planted]).astype(np.float32)
    order = rs.permutation(n)
    return points[order], order >= sheet


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("points", nargs="?", default="", help="scene.pcd or scene.ply")
    parser.add_argument("--synthetic", type=int, default=0, help="a sheet of N points with N // 50 stray ones instead of a scene")
    parser.add_argument("--radius", type=float, default=0.0)
    parser.add_argument("--min_neighbors", type=int, default=3, help="the fewest points within the radius for a normal")
    parser.add_argument("--nb_points", type=int, default=0, help="fewer points than this within the radius: an outlier")
    parser.add_argument("--viewpoint", type=float, nargs=3, default=None)
    parser.add_argument("--out", default="result/normals")
    parser.add_argument("--width", type=int, default=1280)
    parser.add_argument("--height", type=int, default=960)
    flags = parser.parse_args()
    if flags.synthetic > 0:
        points = torch.from_numpy(synthetic(flags.synthetic)[0]).cuda()
        radius, nb_points = flags.radius or SYNTHETIC_RADIUS, flags.nb_points or SYNTHETIC_NB_POINTS
    elif flags.points:
        points, _ = pn2.read_point_cloud(flags.points, want_colors=False)
        radius, nb_points = flags.radius, flags.nb_points or flags.min_neighbors
    else:
        parser.error("a scene file, or --synthetic N")
    if not radius > 0:
        parser.error("--radius")

    nb = pn2.radius_neighborhoods(points, radius, min_neighbors=flags.min_neighbors, viewpoint=flags.viewpoint)
    if nb.status:
        raise ValueError(pn2.neighbors.STATUS_NAMES[nb.status])
    kept, mask = pn2.neighbors.select_by_count(nb.count, nb_points)  # (the counts are there already: no second pass)
    outliers = torch.nonzero(~mask).reshape(-1)
    with_normal = int((nb.count >= flags.min_neighbors).sum())
    print("%d points, %d valid, %d with a normal, at most %d within %g" % (len(points), nb.valid, with_normal, int(nb.count.max()), radius))
    print("%d outliers (fewer than %d points within the radius), %d points kept" % (len(outliers), nb_points, len(kept)))

    os.makedirs(flags.out, exist_ok=True)
    with open(os.path.join(flags.out, "outliers.txt"), "w") as f:
        f.writelines("%d\n" % i for i in outliers.tolist())
    image = pn2.render.render_colors(points, pn2.normal_colors(nb.normals), "top", flags.width, flags.height, size=2)
    pn2.render.write_png(os.path.join(flags.out, "normals.png"), image)
    print("Output written to", flags.out)


if __name__ == "__main__":
    main()
