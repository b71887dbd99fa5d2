"""numpy model of the device-random stream of pn2_dataset_sample (csrc/pn2_dataset.hip), used by the tests only.

Written from the rule the kernel's header documents, not from its mechanism: a sample's scene, centre and angle are three
tagged draws of its counter-based stream, its column is the reference's _extract_z_box (multiscene_ref.column), and from a
column wider than N it keeps the N members with the smallest 64-bit keys, in scene order.  A full sort stands where the
kernel has its four launches.  Every integer is a numpy.uint64 array (multiplication wraps); the centre alone needs a
128-bit product and takes Python ints.

`ds` below is a SemanticDataset; only its host attributes are read (x-sorted scenes, cdf, offsets, label weights, seed)."""
import numpy as np

import multiscene_ref as R

_U = np.uint64
TAG_SCENE = 2 ** 40
TAG_CENTER = TAG_SCENE + 1
TAG_ANGLE = TAG_SCENE + 2


def _u64(x):
    """-> uint64 array of at least one dimension (0-d numpy integers warn where arrays wrap)"""
    if isinstance(x, (int, np.integer)):
        x = [int(x) & 0xFFFFFFFFFFFFFFFF]
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def fmix64(x):
    x = _u64(x)
    x = x ^ (x >> _U(33))
    x = x * _U(0xFF51AFD7ED558CCD)
    x = x ^ (x >> _U(33))
    x = x * _U(0xC4CEB9FE1A85EC53)
    return x ^ (x >> _U(33))


def sample_stream(seed, batch_counter, s):
    """the stream of sample `s` of batch `batch_counter` -> uint64 (1,)"""
    h = fmix64(_u64(seed) + _U(0x9E3779B97F4A7C15))
    h = fmix64(h ^ (_u64(batch_counter) * _U(0xD1B54A32D192ED03) + _U(0x2545F4914F6CDD1D)))
    return fmix64(h ^ (_u64(int(s) & 0xFFFFFFFF) * _U(0xAEF17502108EF2D9) + _U(0x632BE59BD9B4E019)))


def draw64(h, i):
    """draw `i` of stream h: the subset key of the point at scene-local index i, or a tagged per-sample draw"""
    return fmix64(_u64(h) ^ fmix64(_u64(i) + _U(0x8CB92BA72F3D8DD7)))


def unit53(k):
    """the top 53 bits of k as a float64 in [0, 1)"""
    return (_u64(k) >> _U(11)).astype(np.float64) * 2.0 ** -53


def pick_scene(cdf, u):
    """np.random.choice(k, p): the first k with cdf[k] > u, clamped to the last scene"""
    return min(int(np.searchsorted(cdf, u, side="right")), len(cdf) - 1)


def pick_center(k, n):
    """randint(0, n) from a 64-bit draw: the high half of the 128-bit product"""
    return (int(k) * int(n)) >> 64


def pick_subset(h, members, n):
    """members: ascending scene-local indices of the column -> the n indices the batch holds, in output order"""
    cnt = len(members)
    if cnt <= n:
        return members[np.arange(n) % cnt]
    order = np.lexsort((members, draw64(h, members)))  # by key, ties by index
    return np.sort(members[order[:n]])


def rotate_z(p, angle):
    """p @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] written out term by term in float64 (no BLAS, no fused multiply-add)"""
    c, s = np.cos(angle), np.sin(angle)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(x * c + y * (-s)) + z * 0.0, (x * s + y * c) + z * 0.0, (x * 0.0 + y * 0.0) + z * 1.0], 1)


def sample(ds, batch_counter, s, augment=False, scene=None):
    """sample `s` of the batch drawn at `batch_counter`.  scene=None: sample_batch_in_all_files(augment=...); scene=k:
    sample_batch_in_file(k, ...) (the scene is given, nothing is rotated, no weights are looked up).
    -> dict: scene, center (scene-local), cnt, members (scene-local), sel (store indices, (N,)), angle, data (N, 3|6)
    float32, labels (N,) int32, weights (N,) float32, points_raw (N, 3) float64"""
    n = ds.num_points_per_sample
    hx, hy = ds.box_size_x / 2, ds.box_size_y / 2
    h = sample_stream(ds.seed, batch_counter, s)
    in_file = scene is not None
    if not in_file:
        scene = pick_scene(ds.scene_cdf, float(unit53(draw64(h, TAG_SCENE))[0]))
    pts = ds.scene_points[scene]
    center = pick_center(draw64(h, TAG_CENTER)[0], len(pts))
    angle = float((unit53(draw64(h, TAG_ANGLE))[0] * 2.0) * np.pi) if (augment and not in_file) else 0.0
    members = np.nonzero(R.column(pts, pts[center], hx, hy))[0]
    local = pick_subset(h, members, n)
    xyz = R.center_box(pts[local], hx, hy)
    if augment and not in_file:
        xyz = rotate_z(xyz, angle)
    data = xyz.astype(np.float32)
    if ds.use_color:
        data = np.hstack([data, ds.scene_colors[scene][local].astype(np.float32)])
    labels = ds.scene_labels[scene][local].astype(np.uint8).astype(np.int32)
    lw = np.asarray(ds.label_weights, dtype=np.float32)
    weights = np.zeros(n, dtype=np.float32)
    if not in_file:
        weights = np.where(labels < len(lw), lw[np.minimum(labels, len(lw) - 1)], np.float32(0)).astype(np.float32)
    return dict(scene=scene, center=center, cnt=len(members), members=members, angle=angle, data=data, labels=labels,
                sel=(local + int(ds.scene_offsets[scene])).astype(np.int64), weights=weights, points_raw=pts[local])


def batch(ds, batch_counter, batch_size, augment=False, scene=None):
    """the samples of one batch, each field stacked along a leading batch axis (`members` stays a list)"""
    rows = [sample(ds, batch_counter, s, augment, scene) for s in range(batch_size)]
    out = {k: np.array([r[k] for r in rows]) for k in rows[0] if k != "members"}
    out["members"] = [r["members"] for r in rows]
    return out
