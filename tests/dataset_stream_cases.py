"""Scenes, seeds and call plans shared by test_dataset_stream_cpu.py (which asserts that every edge below really occurs)
and test_dataset_stream_gpu.py (which runs them on the device).  Everything is regenerated from seeds; box 10 x 10."""
import numpy as np

import multiscene_ref as R

BOX = 10
N_MAIN = 300            # not a multiple of the 256 threads of the write pass
N_VALUES = (300, 1)     # 1: the threshold bin is the first non-empty one and one candidate is needed
CHUNK = 1024            # slab points per chunk in csrc/pn2_dataset.hip
WORKGROUPS = 64         # workgroups striding over one sample's chunks

SEED_WHOLE, SEED_DIAGONAL, SEED_MIXED, SEED_CHUNKS = 101, 202, 303, 404
WHOLE_BATCHES = (3, 64)
DIAGONAL_BATCHES = (16, 16)
MIXED_BATCHES = (24, 24, 24, 7, 24)  # three consecutive batches, another batch size, the first one again
CHUNKS_BATCH = 16


def whole_counts(n):
    """point counts of the whole-scene store for N = n.  A scene cannot be empty, so N - 1 leaves for N = 1, and equal
    counts (N and 1, N + 1 and 2 N for N = 1) stand once."""
    return sorted({c for c in (1, n - 1, n, n + 1, 2 * n, 1024, 1025, 2048, 2049, 66000) if c > 0})


def whole_scenes(n):
    """extent 3 x 3 under a 10 x 10 box: every column is the whole scene, whatever the centre"""
    return [R.synthetic_scene(1000 + c, c, 3.0, 3.0) + ("whole%d" % c,) for c in whole_counts(n)]


def whole_plan(n):
    """-> [(batch counter, scene, batch size)]: every scene at both batch sizes, one call after the other"""
    calls = [(k, b) for k in range(len(whole_counts(n))) for b in WHOLE_BATCHES]
    return [(ctr, k, b) for ctr, (k, b) in enumerate(calls)]


def diagonal_scene():
    """x uniform over 3 m, y = 40 x / 3 + noise: the slab of any column is the whole scene (x extent < half box), but its
    members lie within |y - yc| <= 5, a contiguous x range of about a quarter of the scene"""
    rs = np.random.RandomState(77)
    n = 20000
    x = rs.uniform(0, 3.0, n)
    pts = np.stack([x, 40.0 * x / 3.0 + rs.normal(0, 0.05, n), np.abs(rs.normal(0, 2.0, n))], 1)
    pts = pts.astype(np.float32).astype(np.float64)
    return pts, rs.randint(0, 9, n).astype(np.int32), rs.randint(0, 256, (n, 3)) / 255.0, "diagonal"


def wide_label_scene():
    """labels over the whole uint8 range: 9 .. 255 have no weight"""
    pts, _, cols = R.synthetic_scene(45, 4000, 15.0, 15.0)
    labels = np.random.RandomState(46).permutation(np.arange(4000) % 256).astype(np.int32)
    return pts, labels, cols, "wide_labels"


def mixed_scenes():
    """dense scenes (columns wider than N), a sparse one (about 150 points per column), one smaller than the box"""
    spec = [(41, 6000, 30.0, 20.0), (42, 2500, 40.0, 40.0), (43, 15000, 25.0, 25.0), (44, 1200, 3.0, 3.0)]
    return [R.synthetic_scene(*s) + ("mixed%d" % i,) for i, s in enumerate(spec)] + [wide_label_scene()]


def chunk_scenes():
    """a scene whose slab is three chunks and one that fits a single chunk (status 5 with max_chunks = 1)"""
    return [R.synthetic_scene(51, 3000, 3.0, 3.0) + ("three_chunks",), R.synthetic_scene(52, 700, 3.0, 3.0) + ("one_chunk",)]


def make(pn2, n, scenes, seed, use_color=True, device="cpu"):
    return pn2.dataset.SemanticDataset(n, "train", use_color, BOX, BOX, "", device=device, seed=seed, scenes=scenes)


def replay_draws(ds):
    """draws for one replayed batch on the mixed store, one sample per scene, each centred on the point nearest the middle
    of its scene; masks select N members at random (seeded).  -> draws, cnt (B,)"""
    n, hx, hy = ds.num_points_per_sample, ds.box_size_x / 2, ds.box_size_y / 2
    rs = np.random.RandomState(9)
    scene = np.arange(ds.num_scenes)
    center, cnt = [], []
    for k in scene:
        p = ds.scene_points[k]
        mid = (p[:, :2].min(0) + p[:, :2].max(0)) / 2
        c = int(np.argmin(((p[:, :2] - mid) ** 2).sum(1)))
        center.append(c)
        cnt.append(int(R.column(p, p[c], hx, hy).sum()))
    masks = np.zeros((len(scene), max(cnt)), dtype=np.uint8)
    for s, c in enumerate(cnt):
        if c > n:
            masks[s, rs.permutation(c)[:n]] = 1
    return dict(scene=scene, center=np.array(center), masks=masks, angle=rs.uniform(0, 2 * np.pi, len(scene))), np.array(cnt)
