"""numpy model of the KITTI frame front end (csrc/pn2_frame.hip, dataset/kitti_dataset.py), used by the tests only.

Written from the rule include/pn2_abi.h documents, not from the kernels' mechanism: the crop keeps a row iff lo <= p <= hi on
every axis in float64, inclusive, in frame order; the sort is stable by x; a frame of at most N points is repeated (j mod cnt),
a larger one keeps the set positions of the replayed mask or, in device mode, the N members with the smallest 64-bit keys
draw64(sample_stream(seed, counter, 0), i), ties broken by index, in ascending order; centring subtracts (min_x + bx / 2,
min_y + by / 2, min_z) of the SAMPLED points in float64 and rounds once to float32.  A full sort stands where the kernel has its
histogram.  tests/golden/kitti_frames.npz pins this model to the reference's own code (tests/golden/make_kitti_golden.py)."""
import numpy as np

from dataset_stream_ref import draw64, sample_stream

MIN_Z, MAX_Z = -2, 5  # kitti_dataset.py:15-16
ST_OK, ST_MASK = 0, 3


def kitti_box(box_size_x, box_size_y):
    """-> lo (3,), hi (3,) float64 of KittiFileData.__init__ :15-20"""
    return (np.array([-box_size_x / 2.0, -box_size_y / 2.0, MIN_Z], dtype=np.float64),
            np.array([box_size_x / 2.0, box_size_y / 2.0, MAX_Z], dtype=np.float64))


def crop(frame, lo, hi):
    """frame (n, >=3) float32 -> points (cnt,3) float64 in frame order, src (cnt,) int32 frame rows"""
    p = np.asarray(frame)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.all((p >= lo) & (p <= hi), axis=1)
    src = np.nonzero(keep)[0].astype(np.int32)
    return p[src], src


def stable_order(points):
    """the permutation of the x-sort: ties keep their order"""
    return np.argsort(points[:, 0], kind="stable")


def file_data(frame, box_size_x, box_size_y):
    """KittiFileData.__init__ -> points (cnt,3) float64 x-sorted, source_index (cnt,) int32"""
    p, src = crop(frame, *kitti_box(box_size_x, box_size_y))
    order = stable_order(p)
    return p[order], src[order]


def select(cnt, npts, mask=None, seed=0, counter=0):
    """-> sel (npts,) int32, status"""
    if cnt <= npts:
        return (np.arange(npts) % cnt).astype(np.int32), ST_OK
    if mask is not None:
        sel = np.nonzero(np.asarray(mask))[0].astype(np.int32)
        return (sel, ST_OK) if len(sel) == npts else (np.zeros(npts, np.int32), ST_MASK)
    idx = np.arange(cnt, dtype=np.uint64)
    keys = draw64(sample_stream(seed, counter, 0), idx)
    order = np.lexsort((idx, keys))  # by key, ties by index
    return np.sort(order[:npts]).astype(np.int32), ST_OK


def center(points, box_size_x, box_size_y):
    """_center_box (semantic_dataset.py:109-121) -> float64"""
    box_min = np.min(points, axis=0)
    shift = np.array([box_min[0] + box_size_x / 2, box_min[1] + box_size_y / 2, box_min[2]])
    return points - shift


def sample(points, npts, box_size_x, box_size_y, mask=None, seed=0, counter=0):
    """pn2_frame_sample -> sel (npts,) int32, centered (npts,3) float32, raw (npts,3) float64, status"""
    sel, status = select(len(points), npts, mask, seed, counter)
    if status != ST_OK:
        return sel, np.zeros((npts, 3), np.float32), np.zeros((npts, 3), np.float64), status
    raw = points[sel]
    return sel, center(raw, box_size_x, box_size_y).astype(np.float32), raw, status


def tie_frame(seed=5, n=600):
    """a frame whose x takes 24 values only (and both zeros): many ties"""
    rs = np.random.RandomState(seed)
    x = (rs.randint(-12, 12, n) / 4.0).astype(np.float32)
    x[rs.random_sample(n) < 0.05] = -0.0
    return np.stack([x, rs.uniform(-6, 6, n).astype(np.float32), rs.uniform(-3, 6, n).astype(np.float32),
                     rs.random_sample(n).astype(np.float32)], 1)
