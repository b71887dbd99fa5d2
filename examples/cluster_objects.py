"""Group the labelled points of a scene into objects on one MI355X: which points form one car, and how many cars there are.

    python examples/cluster_objects.py --points scene.pcd --labels scene.labels --eps 0.5 --classes 8 --min_points 10 --out result
    python examples/cluster_objects.py --synthetic 3000 --eps 0.2 --out result
    python examples/cluster_objects.py --points frame.pcd --labels frame.labels --eps 0.5 --ground 0.2 --out result

The cloud and the labels are read on the device (pn2.read_point_cloud, pn2.load_labels), the points of each class in --classes
(every label >= 1 that occurs when it is not given) are clustered with pn2.euclidean_clusters -- two points in one object when a
chain of points of their label joins them in steps of at most --eps -- and the result is written to
    <out>/objects.txt   one line per object: id label size min_x min_y min_z max_x max_y max_z (repr-exact floats)
    <out>/objects.png   the scene from above, every object in a colour of its own, everything else grey (pn2.render)
with one line per class and its object count on the terminal.  --synthetic N makes N points in tight blobs of known sizes on a
lattice (synthetic(N) below), so the expected output is known.
--boxes describes every object as well (pn2.describe_clusters, upright: the box turns about the z axis only): each object's line
gains nine columns, center_x center_y center_z (the box centre) length width height (the box edges along its axes) yaw (radians,
the heading of the long axis) centroid_x centroid_y (repr-exact floats), and
    <out>/boxes.png     objects.png with every object's box drawn around it in the object's colour (pn2.box_wireframe)
is written too.
--ground THR takes the ground out first: pn2.segment_plane with the axis (0,0,1) and a normal within 15 degrees of it
(--ground-trials hypotheses), its inliers are left out of the clustering, and objects.txt begins with the line
    ground count a b c d                        the exact, unnormalised plane a*x + b*y + c*z + d = 0 (repr-exact floats)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

SYNTHETIC_EPS = 0.2
GROUND_MAX_ANGLE = 15.0  # degrees between the ground's normal and the z axis, at the most


def synthetic(n, seed=0):
    """-> points (n,3) float32, labels (n,) int32: blobs of 1 + (37 k mod 60) points, each inside a cube of side 0.1 (any two of
    its points are closer than SYNTHETIC_EPS) at the lattice site (k mod 16, k div 16, 0) (two blobs are at least 0.9 apart);
    blob k has label 1 + k mod 3; the rows are shuffled."""
    rs = np.random.RandomState(seed)
    blob, k = [], 0
    while len(blob) < n:
        blob += [k] * min(1 + (37 * k) % 60, n - len(blob))
        k += 1
    blob = np.array(blob)
    site = np.stack([blob % 16, blob // 16, np.zeros_like(blob)], 1).astype(np.float64)
    points = (site + rs.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)
    labels = (1 + blob % 3).astype(np.int32)
    order = rs.permutation(n)
    return points[order], labels[order]


def object_lines(clusters):
    """-> the lines of objects.txt"""
    rows = zip(clusters.label.tolist(), clusters.size.tolist(), clusters.bbox.cpu().numpy())
    return ["%d %d %d %s" % (i, label, size, " ".join(repr(float(v)) for v in box)) for i, (label, size, box) in enumerate(rows)]


def box_columns(boxes):
    """-> per object the columns --boxes appends to its line of objects.txt"""
    rows = torch.cat([boxes.center, boxes.extent, boxes.yaw()[:, None], boxes.centroid[:, :2]], 1).cpu().numpy()
    return [" ".join(repr(float(v)) for v in row) for row in rows]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--points", default="", help="scene.pcd or scene.ply")
    parser.add_argument("--labels", default="", help="scene.labels: one label per point")
    parser.add_argument("--synthetic", type=int, default=0, help="N points in blobs on a lattice instead of a scene")
    parser.add_argument("--eps", type=float, default=0.0, help="the largest step between two points of one object")
    parser.add_argument("--classes", type=int, nargs="*", default=None, help="the labels to cluster (default: every label >= 1)")
    parser.add_argument("--min_points", type=int, default=1)
    parser.add_argument("--max_points", type=int, default=0, help="0: no upper bound")
    parser.add_argument("--ground", type=float, default=0.0, help="remove the ground first: points within this distance of it")
    parser.add_argument("--ground-trials", type=int, default=1024, help="RANSAC hypotheses for --ground")
    parser.add_argument("--boxes", action="store_true", help="describe every object: oriented box columns and boxes.png")
    parser.add_argument("--out", default="result/objects")
    parser.add_argument("--width", type=int, default=1280)
    parser.add_argument("--height", type=int, default=960)
    flags = parser.parse_args()
    if flags.synthetic > 0:
        points, labels = (torch.from_numpy(a).cuda() for a in synthetic(flags.synthetic))
        eps = flags.eps or SYNTHETIC_EPS
    elif flags.points and flags.labels:
        points, _ = pn2.read_point_cloud(flags.points, want_colors=False)
        labels = pn2.load_labels(flags.labels)
        if len(points) != len(labels):
            raise ValueError("len(points) != len(labels)")
        eps = flags.eps
    else:
        parser.error("--points and --labels, or --synthetic N")
    if not eps > 0:
        parser.error("--eps")
    classes = flags.classes if flags.classes else [c for c in torch.unique(labels).tolist() if c >= 1]
    ground_lines = []
    if flags.ground > 0:
        ground = pn2.segment_plane(points, flags.ground, trials=flags.ground_trials, axis=(0, 0, 1), max_angle=GROUND_MAX_ANGLE)
        labels = torch.where(ground.inliers, torch.full_like(labels, -1), labels)
        ground_lines = ["ground %d %s" % (ground.count, " ".join(repr(v) for v in ground.raw.tolist()))]
        print("ground: %d of %d points" % (ground.count, len(points)))

    clusters = pn2.euclidean_clusters(points, eps, labels=labels, classes=classes, min_points=flags.min_points,
                                      max_points=flags.max_points)
    per_class = torch.bincount(clusters.label, minlength=max(classes) + 1).tolist() if clusters.count else []
    for c in classes:
        print("class %d: %d objects" % (c, per_class[c] if c < len(per_class) else 0))
    print("%d objects, %d of %d points in one" % (clusters.count, int((clusters.ids >= 0).sum()), len(points)))

    lines = object_lines(clusters)
    boxes = None
    if flags.boxes:
        boxes = pn2.describe_clusters(points, clusters, upright=True)
        lines = [line + " " + more for line, more in zip(lines, box_columns(boxes))]

    os.makedirs(flags.out, exist_ok=True)
    with open(os.path.join(flags.out, "objects.txt"), "w") as f:
        f.writelines(line + "\n" for line in ground_lines + lines)
    colors = pn2.cluster_colors(clusters.ids)
    renderer = pn2.render.Renderer(flags.width, flags.height, 2, device=points.device)
    view = pn2.render.fit_view(points, "top", flags.width, flags.height)
    image = pn2.render.render_colors(points, colors, view, renderer=renderer)
    pn2.render.write_png(os.path.join(flags.out, "objects.png"), image)
    if boxes is not None:  # the same z-buffer: the edges go in behind the cloud's indices, in their objects' colours
        edges, owner = pn2.box_wireframe(boxes)
        renderer.splat(edges, view, index0=len(points))
        image = renderer.image(torch.cat([colors, pn2.cluster_colors(owner)]))
        pn2.render.write_png(os.path.join(flags.out, "boxes.png"), image)
    print("Output written to", flags.out)


if __name__ == "__main__":
    main()
