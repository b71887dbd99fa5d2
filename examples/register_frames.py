"""Frames of one scene laid onto each other on one MI355X: rigid registration (ICP) of every frame to the one before it, the
poses composed, and the frames merged into one map.

    python examples/register_frames.py --synthetic --out result
    python examples/register_frames.py frame0.pcd frame1.pcd frame2.pcd --max_distance 0.5 --out result

Frame k is aligned to frame k-1 with pn2.registration_icp, once point-to-point and once point-to-plane (the target's normals
from pn2.estimate_normals); the relative motions are composed into each frame's pose in the coordinates of frame 0, every frame
is moved there with pn2.transform_points, and the merged cloud is written to
    <out>/map.png    the map from above, every frame in a colour of its own (pn2.render)
with iterations, fitness, rmse and -- for --synthetic, where the motions are known -- the pose error per frame on the terminal.
--synthetic makes a scene of a floor, two walls and three boxes, and three frames of it: each a random subsample seen from a
pose of its own (synthetic(N) below)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

FRAME_COLORS = ((230, 80, 60), (70, 200, 90), (80, 120, 240), (230, 200, 60), (200, 80, 220), (60, 210, 210))
SYNTHETIC_MAX_DISTANCE = 0.4
SYNTHETIC_NORMAL_RADIUS = 0.5


def _rigid(axis, degrees, translation):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    T[:3, 3] = translation
    return T


def _box_faces(rs, m, lo, hi):
    """m points on the five visible faces of the box [lo, hi] standing on the floor"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    p = lo + rs.uniform(0, 1, (m, 3)) * (hi - lo)
    face = rs.randint(0, 5, m)
    for f, (axis, side) in enumerate(((0, lo), (0, hi), (1, lo), (1, hi), (2, hi))):
        p[face == f, axis] = side[axis]
    return p


def synthetic(n, seed=0):
    """-> frames: three (n,3) float32 clouds, poses: three 4x4 -- frame k holds n points of the scene (a 8 x 8 floor, two walls
    2.5 high, three boxes), drawn afresh for every frame, in the coordinates of a sensor at poses[k] (poses[0] = identity):
    scene point = poses[k] @ frame point."""
    rs = np.random.RandomState(seed)
    poses = [np.eye(4), _rigid([0.1, -0.2, 1.0], 2.0, [0.15, -0.1, 0.02]), _rigid([-0.1, 0.1, 1.0], 4.5, [0.3, -0.15, 0.05])]
    frames = []
    for pose in poses:
        parts = n * np.array([0.4, 0.15, 0.15, 0.1, 0.1]) // 1
        parts = [int(v) for v in parts] + [n - int(parts.sum())]
        floor = np.concatenate([rs.uniform(0, 8, (parts[0], 2)), np.zeros((parts[0], 1))], 1)
        wall_x = np.stack([np.zeros(parts[1]), rs.uniform(0, 8, parts[1]), rs.uniform(0, 2.5, parts[1])], 1)
        wall_y = np.stack([rs.uniform(0, 8, parts[2]), np.full(parts[2], 8.0), rs.uniform(0, 2.5, parts[2])], 1)
        boxes = [_box_faces(rs, parts[3], (2, 2, 0), (3.5, 3, 1.2)), _box_faces(rs, parts[4], (5, 4.5, 0), (6, 6.5, 1.6)),
                 _box_faces(rs, parts[5], (1.5, 5.5, 0), (2.5, 6.5, 0.8))]
        scene = np.concatenate([floor, wall_x, wall_y] + boxes) + [-4.0, -4.0, -1.5]  # the sensor above the middle of the floor
        inv = np.linalg.inv(pose)
        frames.append((scene @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    return frames, poses


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("frames", nargs="*", help="two or more .pcd / .ply files, in order")
    parser.add_argument("--synthetic", action="store_true", help="three frames of a made-up scene instead of files")
    parser.add_argument("--points", type=int, default=20000, help="points per synthetic frame")
    parser.add_argument("--max_distance", type=float, default=0.0, help="the largest distance of a correspondence")
    parser.add_argument("--normal_radius", type=float, default=0.0, help="the radius of the normals (default 1.25 x max_distance)")
    parser.add_argument("--max_iteration", type=int, default=30)
    parser.add_argument("--out", default="result/frames")
    parser.add_argument("--width", type=int, default=1280)
    parser.add_argument("--height", type=int, default=960)
    flags = parser.parse_args()
    truth = None
    if flags.synthetic:
        host, truth = synthetic(flags.points)
        frames = [torch.from_numpy(f).cuda() for f in host]
        max_distance = flags.max_distance or SYNTHETIC_MAX_DISTANCE
        normal_radius = flags.normal_radius or SYNTHETIC_NORMAL_RADIUS
    elif len(flags.frames) >= 2:
        frames = [pn2.read_point_cloud(path, want_colors=False)[0] for path in flags.frames]
        max_distance, normal_radius = flags.max_distance, flags.normal_radius or 1.25 * flags.max_distance
    else:
        parser.error("two or more frame files, or --synthetic")
    if not max_distance > 0:
        parser.error("--max_distance")

    poses = {"point_to_point": [np.eye(4)], "point_to_plane": [np.eye(4)]}
    for k in range(1, len(frames)):
        normals = pn2.estimate_normals(frames[k - 1], normal_radius, viewpoint=(0, 0, 0))
        for estimation, chain in poses.items():
            reg = pn2.registration_icp(frames[k], frames[k - 1], max_distance, estimation=estimation, max_iteration=flags.max_iteration,
                                       target_normals=normals if estimation == "point_to_plane" else None)
            if reg.status:
                raise ValueError("frame %d: %s" % (k, pn2.icp.STATUS_NAMES[reg.status]))
            chain.append(pn2.icp.compose(chain[-1], reg.transformation))  # frame k -> frame k-1 -> ... -> frame 0
            line = "frame %d %s: %d iterations, fitness %.3f, rmse %.4f" % (k, estimation, reg.iterations, reg.fitness, reg.inlier_rmse)
            if truth is not None:
                line += ", pose error %.4f deg, %.4f units" % pn2.icp.rigid_error(chain[-1], truth[k])
            print(line)

    merged = torch.cat([pn2.transform_points(f, T) for f, T in zip(frames, poses["point_to_plane"])])
    colors = torch.cat([torch.tensor(FRAME_COLORS[k % len(FRAME_COLORS)], dtype=torch.uint8, device=merged.device).repeat(len(f), 1)
                        for k, f in enumerate(frames)])
    os.makedirs(flags.out, exist_ok=True)
    image = pn2.render.render_colors(merged, colors, "top", flags.width, flags.height, size=2)
    pn2.render.write_png(os.path.join(flags.out, "map.png"), image)
    print("%d points of %d frames merged; output written to %s" % (len(merged), len(frames), flags.out))


if __name__ == "__main__":
    main()
