"""Pins tests/frame_ref.py to the REFERENCE's own KITTI frame code and freezes the result (run where the reference checkout
exists):

    python tests/golden/make_kitti_golden.py      -> tests/golden/kitti_frames.npz

dataset/kitti_dataset.py and dataset/semantic_dataset.py cannot be imported (open3d, pykitti), so SemanticFileData and
KittiFileData are lifted out of the reference's source files with `ast` -- unmodified, never copied into this repository -- and
executed with stand-ins: open3d.PointCloud / Vector3dVector become a float64 array, crop_point_cloud becomes the project's
inclusive rule (lo <= p <= hi on every axis; Open3D itself is not available to pin it), and np.random is seen through a recorder,
so the shuffled sample mask is stored and the device sampler can replay it.

Cases: the cropped count below N, equal to N, N + 1 and several times N, for N = 16 and N = 1024; frames have 4 columns.  The
kept rows of every frame have pairwise distinct float32 x, so np.argsort and the stable rule give the same order."""
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_DS = "/root/reference/dataset/semantic_dataset.py"
REF_KITTI = "/root/reference/dataset/kitti_dataset.py"

import frame_ref as F  # noqa: E402


def lift(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), (path, names)
    exec(compile(ast.fix_missing_locations(ast.Module(body=keep, type_ignores=[])), path, "exec"), ns)
    return ns


class MaskRecorder:
    """np.random stand-in: shuffles with the global numpy stream and keeps what came out"""

    def __init__(self):
        self.masks = []

    def shuffle(self, x):
        np.random.shuffle(x)
        self.masks.append(np.array(x, dtype=np.uint8))


class RecordingNumpy(types.ModuleType):
    """`np` for the lifted code: numpy itself, except np.random, which is the recorder"""

    def __init__(self, rec):
        super().__init__("np")
        self.random = rec

    def __getattr__(self, k):
        return getattr(np, k)


class _PointCloud:
    points = None


def _crop_point_cloud(pcd, lo, hi):
    out = _PointCloud()
    p = pcd.points
    out.points = p[np.all((p >= np.asarray(lo, dtype=np.float64)) & (p <= np.asarray(hi, dtype=np.float64)), axis=1)]
    return out


def lifted_reference(rec):
    npx = RecordingNumpy(rec)
    o3d = types.SimpleNamespace(PointCloud=_PointCloud, Vector3dVector=lambda a: np.array(a, dtype=np.float64),
                                crop_point_cloud=_crop_point_cloud)
    ns = lift(REF_DS, ["SemanticFileData"], {"np": npx, "os": os, "open3d": o3d})
    return lift(REF_KITTI, ["KittiFileData"], dict(ns, open3d=o3d))["KittiFileData"]


def make_frame(rs, inside, outside, bx, by):
    """(inside + outside, 4) float32: `inside` rows in the box with pairwise distinct x, `outside` rows beyond one bound, mixed"""
    x = rs.permutation(8 * inside)[:inside].astype(np.float64) / (8 * inside) * bx - bx / 2 + bx / (32.0 * inside)
    p = np.stack([x, rs.uniform(-by / 2, by / 2, inside), rs.uniform(F.MIN_Z, F.MAX_Z, inside)], 1)
    q = np.stack([rs.uniform(-bx, bx, outside), rs.uniform(-by, by, outside), rs.uniform(-4, 8, outside)], 1)
    axis = rs.randint(0, 3, outside)
    far = np.array([bx, by, 10.0])[axis] * rs.choice([-1.0, 1.0], outside)
    q[np.arange(outside), axis] = far  # beyond the box on one axis at least
    rows = np.concatenate([p, q])[rs.permutation(inside + outside)]
    return np.concatenate([rows, rs.random_sample((len(rows), 1))], 1).astype(np.float32)


# (N, cropped count, rows outside the box, box_size_x, box_size_y, seed)
CASES = [(16, 7, 9, 10, 10, 0), (16, 16, 11, 10, 10, 1), (16, 17, 30, 10, 10, 2), (16, 200, 77, 10, 10, 3),
         (1024, 300, 211, 12, 8, 4), (1024, 1024, 500, 12, 8, 5), (1024, 1025, 333, 12, 8, 6), (1024, 4100, 2000, 12, 8, 7)]


def main():
    out = {}
    for ci, (n, inside, outside, bx, by, seed) in enumerate(CASES):
        rs = np.random.RandomState(1000 + seed)
        frame = make_frame(rs, inside, outside, bx, by)
        rec = MaskRecorder()
        Ref = lifted_reference(rec)
        np.random.seed(seed)
        ref = Ref(frame[:, :3], bx, by)  # KittiDataset passes points_with_intensity[:, :3] (:96)
        centered, raw = ref.get_batch_of_one_z_box_from_origin(n)
        assert len(ref.points) == inside, (len(ref.points), inside)
        assert len(np.unique(ref.points[:, 0].astype(np.float32))) == inside, "kept rows must have pairwise distinct float32 x"
        assert centered.dtype == np.float64 and centered.shape == (1, n, 3) and raw.shape == (1, n, 3)
        assert len(rec.masks) == (1 if inside > n else 0)
        mask = rec.masks[0] if rec.masks else np.zeros(0, dtype=np.uint8)
        # the model, on the same frame and the recorded mask
        pts, src = F.file_data(frame, bx, by)
        assert pts.dtype == np.float64 and np.array_equal(pts.view(np.int64), ref.points.view(np.int64)), "x-sorted frame differs"
        assert np.array_equal(frame[src, :3].astype(np.float64).view(np.int64), pts.view(np.int64))
        sel, cen, mraw, status = F.sample(pts, n, bx, by, mask=mask if inside > n else None)
        assert status == 0 and np.array_equal(mraw.view(np.int64), raw[0].view(np.int64)), "raw batch differs"
        assert np.array_equal(cen.view(np.int32), centered[0].astype(np.float32).view(np.int32)), "centred batch differs"
        lo = centered[0].min(axis=0)
        assert np.allclose(lo, [-bx / 2, -by / 2, 0], atol=1e-12), lo
        tag = "c%d_" % ci
        out[tag + "meta"] = np.array([n, inside, bx, by, seed])
        out[tag + "frame"] = frame
        out[tag + "source_index"] = src
        out[tag + "mask"] = mask
        out[tag + "sel"] = sel
        out[tag + "centered"] = centered  # float64, as the reference returns it; the network is fed its float32 cast
        out[tag + "raw"] = raw
        print("case %d: N %d frame %d cropped %d box %dx%d mask %d" % (ci, n, len(frame), inside, bx, by, len(mask)))
    out["num_cases"] = np.array(len(CASES))
    path = os.path.join(ROOT, "tests", "golden", "kitti_frames.npz")
    np.savez_compressed(path, **out)
    print("model == lifted reference on %d cases; %s: %d bytes" % (len(CASES), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
