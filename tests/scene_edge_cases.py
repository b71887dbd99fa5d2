"""Inputs and numpy models shared by test_scene_edges_cpu.py (which asserts from the model alone that every edge below really
occurs) and test_scene_edges_gpu.py (which runs the cases on the device): csrc/pn2_scene.hip at its edges, voxel down-sampling
(A) and the single-scene sampler (B).  Everything is regenerated from seeds; nothing is stored.

The model is oracle/dataset_oracle.py: voxel_down_sample, and FileDataOracle's _extract_z_box, _center_box and the repeat branch
of _get_fix_sized_sample_mask.  Added here only: the voxel index of a point (the oracle's own expression), and the gather of
a column through a GIVEN mask, which the oracle draws from np.random."""
import numpy as np

from oracle.dataset_oracle import FileDataOracle, voxel_down_sample

BITS = 21
LIMIT = 1 << BITS  # voxel indices per axis: 21 bits each in the 63-bit sort key

# ======================================================================================================================
# A. voxel down-sampling
# ======================================================================================================================


def _attrs(rs, n):
    """colours k / 255 and labels 1 .. 8 (no label 0: nothing is skipped)"""
    return rs.randint(0, 256, (n, 3)) / 255.0, rs.randint(1, 9, n).astype(np.int32)


def voxel_index(points, vs):
    """the oracle's voxel index (dataset_oracle.py: min_bound, floor of the true division), (n,3) int64"""
    points = np.asarray(points, dtype=np.float64)
    min_bound = points.min(axis=0) - vs * 0.5
    return np.floor((points - min_bound) / vs).astype(np.int64)


def voxel_model(points, colors, labels, vs, skip_label_zero=True):
    """what down_sample_arrays must return: label 0 dropped first (when labels exist), then the oracle"""
    if labels is not None and skip_label_zero:
        keep = np.asarray(labels) != 0
        points, labels = points[keep], labels[keep]
        colors = None if colors is None else colors[keep]
    return voxel_down_sample(points, colors, labels, vs)


# ---- A1: voxel faces -------------------------------------------------------------------------------------------------
FACE_VS = (0.05, 0.1, 0.25)
FACE_ORIGINS = (0.0, -312.75, 1000.0)
FACE_TRIPLES, FACE_POINTS, FACE_J = 2000, 3999, 12000
FACE_SEED = 1


def face_cloud(vs, origin, seed=FACE_SEED):
    """p = origin + (j - 0.5) vs per axis, j integer in [1, 12000), and one point at the origin: min_bound = origin - vs / 2, so
    (p - min_bound) / vs is j up to rounding -- every coordinate sits on a voxel face.  2000 triples of j, each at least once,
    3999 rows: voxels have about two members.  -> points (4000,3), j (4000,3) (0 for the origin row), colours, labels"""
    rs = np.random.RandomState(seed)
    triples = rs.randint(1, FACE_J, (FACE_TRIPLES, 3))
    rows = np.concatenate((np.arange(FACE_TRIPLES), rs.randint(0, FACE_TRIPLES, FACE_POINTS - FACE_TRIPLES)))
    j = triples[rs.permutation(rows)]
    pts = origin + (j - 0.5) * vs
    at = FACE_POINTS // 2  # the origin row in the middle of the input
    pts = np.concatenate((pts[:at], np.full((1, 3), float(origin)), pts[at:]))
    j = np.concatenate((j[:at], np.zeros((1, 3), dtype=j.dtype), j[at:]))
    cols, labels = _attrs(rs, len(pts))
    return pts, j, cols, labels


def face_counts(pts, j, vs):
    """over the 3 x 3999 lattice coordinates: how many quotients are exact integers, have a floor below j, a floor that the
    reciprocal multiplication changes, a floor that a float32 quotient changes"""
    lattice = j[:, 0] > 0
    mb = pts.min(axis=0) - vs * 0.5
    p, jj = pts[lattice], j[lattice]
    q = (p - mb) / vs
    fl = np.floor(q)
    recip = np.floor((p - mb) * (1.0 / vs))
    q32 = (p.astype(np.float32) - mb.astype(np.float32)) / np.float32(vs)
    assert q32.dtype == np.float32
    return dict(integer=int((q == fl).sum()), below=int((fl < jj).sum()), reciprocal=int((recip != fl).sum()),
                float32=int((np.floor(q32).astype(np.float64) != fl).sum()), total=q.size)


# ---- A2: sum order ---------------------------------------------------------------------------------------------------
SUM_SEED = 0
SUM_MEMBERS, SUM_MEMBERS_WIDE, SUM_SINGLES = 3001, 20000, 5000


def _decades(rs, n):
    """magnitudes over ten decades, all inside [0, 0.04)"""
    return rs.uniform(0, 1, (n, 3)) * 10.0 ** rs.randint(-9, 1, (n, 3)) * 0.04


def sum_order_cloud(members, singles=0, seed=SUM_SEED):
    """voxel_size 1.0: `members` points inside one voxel (all within [0, 0.04)^3, min_bound >= -0.5) whose float64 sum depends
    on the order, colours likewise; `singles` voxels of one member each further along x, interleaved in the input"""
    rs = np.random.RandomState(seed)
    pts, cols = _decades(rs, members), _decades(rs, members)
    if singles:
        one = np.stack((1.7 + np.arange(singles), np.full(singles, 0.02), np.full(singles, 0.02)), 1)
        order = rs.permutation(members + singles)
        pts = np.concatenate((pts, one))[order]
        cols = np.concatenate((cols, _decades(rs, singles)))[order]
    labels = rs.randint(1, 9, len(pts)).astype(np.int32)
    return pts, cols, labels


# ---- A3: counts ------------------------------------------------------------------------------------------------------
COUNTS_SMALL = (1, 2, 255, 256, 257, 1023, 1024, 1025)
COUNTS_LARGE = (262143, 262144, 262145)  # 256 threads x the 1024-workgroup cap of voxel_minmax_kernel, -1 / +1
COUNT_VS = 0.05


def count_cloud(n):
    rs = np.random.RandomState(7000 + n % 1000 + n // 1000)
    if n == 2:
        pts = np.repeat(rs.uniform(-3, 3, (1, 3)), 2, axis=0)  # the same point twice
    elif n <= 1025:
        side = max(1, int(round((n / 4.0) ** (1.0 / 3.0))))  # about four members per voxel
        pts = rs.uniform(0, COUNT_VS * side, (n, 3))
    else:
        pts = rs.uniform(-3, 3, (n, 3))
    cols, labels = _attrs(rs, n)
    return pts, cols, labels


# ---- A4: order of the output ------------------------------------------------------------------------------------------
ORDER_VS = 0.05
ORDER_INDICES = [(0, 0, 0), (5, 7, 9), (5, 7, 10), (5, 8, 9), (6, 7, 9), (5, 7, LIMIT - 1), (5, LIMIT - 1, 9), (5, LIMIT - 1, 10),
                 (LIMIT - 1, 0, 0), (LIMIT - 1, 7, 9), (LIMIT - 1, 7, 10), (LIMIT - 1, LIMIT - 1, LIMIT - 1), (LIMIT - 2, LIMIT - 1, 0),
                 (1, 0, LIMIT - 1), (0, 1, 0), (0, 0, 1), (1, 0, 0)]


def order_cloud():
    """points in the middle of the voxels ORDER_INDICES (p = index * vs, min_bound = -vs / 2), two or three members each,
    shuffled: the output must come sorted by (ix, iy, iz), and ix = 2^21 - 1 sets bit 62 of the key"""
    rs = np.random.RandomState(40)
    ind = np.array(ORDER_INDICES, dtype=np.float64)
    reps = np.concatenate((np.arange(len(ind)), np.arange(len(ind)), rs.randint(0, len(ind), len(ind))))
    reps = reps[rs.permutation(len(reps))]
    pts = ind[reps] * ORDER_VS + rs.uniform(0, 0.3, (len(reps), 3)) * ORDER_VS  # quotient in [index + 0.5, index + 0.8)
    pts = np.concatenate((pts[:9], np.zeros((1, 3)), pts[9:]))  # the minimum is 0 on every axis
    cols, labels = _attrs(rs, len(pts))
    return pts, cols, labels, np.concatenate((reps[:9], [0], reps[9:]))


# ---- A5: the 21-bit limit ---------------------------------------------------------------------------------------------
LIMIT_VS = 0.05
EXTENT_FITS = LIMIT_VS * (LIMIT - 1.5)   # largest index 2^21 - 1
EXTENT_OVER = LIMIT_VS * (LIMIT - 0.5)   # largest index 2^21


def limit_cloud(axis, extent):
    pts = np.zeros((2, 3))
    pts[1, axis] = extent
    return pts, np.array([[0.25, 0.5, 0.75], [1.0, 0.0, 0.125]]), np.array([3, 4], dtype=np.int32)


# ---- A6: labels -------------------------------------------------------------------------------------------------------
LABEL_VS = 1.0


def label_cloud():
    """voxel 0 (x in [0, 0.5)): labels 5 3 5 3 -> the tie goes to 3; voxel 1: 63 1 63 -> 63; voxel 2: 8; voxel 3: 1 2 2 -> 2"""
    x = np.array([0.0, 0.1, 0.2, 0.3, 1.1, 1.2, 1.3, 2.2, 3.1, 3.2, 3.3])
    labels = np.array([5, 3, 5, 3, 63, 1, 63, 8, 1, 2, 2], dtype=np.int32)
    pts = np.stack((x, np.linspace(0.0, 0.3, len(x)), np.linspace(0.3, 0.0, len(x))), 1)
    cols = np.random.RandomState(60).randint(0, 256, (len(x), 3)) / 255.0
    return pts, cols, labels


# ---- A7: signed zero and tiny values ----------------------------------------------------------------------------------
TINY = np.float64(5e-324)  # the smallest subnormal


def signed_zero_cloud():
    """the minimum is -0.0 on x (with +0.0 rows beside it) and +0.0 on y and z; a voxel of zeros of both signs"""
    pts = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, 0.04, 0.0], [0.3, 0.0, 0.01], [-0.0, 0.31, 0.0], [0.31, 0.3, 0.3],
                    [0.0, -0.0, -0.0]])
    cols, labels = _attrs(np.random.RandomState(70), len(pts))
    return pts, cols, labels


def subnormal_cloud():
    """subnormal coordinates (sums and means stay subnormal: one voxel at voxel_size 0.05) beside ordinary ones"""
    rs = np.random.RandomState(71)
    tiny = rs.randint(0, 1000, (7, 3)) * TINY
    tiny[0] = 0.0
    pts = np.concatenate((tiny, rs.uniform(0.1, 0.5, (9, 3)), np.array([[2.0 ** -1030, 2.0 ** -1040, 3 * TINY]])))
    cols, labels = _attrs(rs, len(pts))
    cols[:7] = rs.randint(0, 1000, (7, 3)) * TINY
    return pts, cols, labels


# ---- A8 / A9: an ordinary cloud ---------------------------------------------------------------------------------------
PLAIN_N, PLAIN_VS = 1000, 0.25
NONFINITE_ROWS = (0, PLAIN_N // 2, PLAIN_N - 1)
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)


def plain_cloud(n=PLAIN_N, seed=80):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-3, 3, (n, 3))
    cols, labels = _attrs(rs, n)
    return pts, cols, labels


# ======================================================================================================================
# B. the single-scene sampler
# ======================================================================================================================
BOX = 10
HALF = BOX / 2.0


def oracle_of(scene):
    pts, labels, cols = scene
    return FileDataOracle(pts, np.zeros(len(pts), dtype=np.int32) if labels is None else labels,
                          np.zeros_like(pts) if cols is None else cols, BOX, BOX)


def slab(o, ci):
    """[i_min, i_max) of the column around sorted point ci, as _extract_z_box searches it"""
    c = o.points[ci]
    return int(np.searchsorted(o.points[:, 0], c[0] - HALF)), int(np.searchsorted(o.points[:, 0], c[0] + HALF))


def column(o, ci):
    """scene indices of the column around sorted point ci, in scene order"""
    return np.flatnonzero(o._extract_z_box(o.points[ci]))


def sample_model(o, ci, mask_row, npts):
    """one sample: the column, the given mask (cnt > npts) or the oracle's repeat branch, the gathers, _center_box, the casts"""
    idx = column(o, ci)
    cnt = len(idx)
    if cnt > npts:
        pick = np.asarray(mask_row[:cnt]) != 0
        assert pick.sum() == npts
        sel = idx[pick]
    else:
        sel = idx[o._get_fix_sized_sample_mask(o.points[idx], npts)]  # no random draw on this branch
    raw = o.points[sel]
    return dict(idx=idx, cnt=cnt, sel=sel, raw=raw, centered=o._center_box(raw).astype(np.float32),
                labels=o.labels[sel].astype(np.int32), colors=o.colors[sel].astype(np.float32))


def random_masks(o, centers, npts, cap, seed):
    """(b, cap) uint8: for every column wider than npts a seeded random choice of exactly npts of its members"""
    rs = np.random.RandomState(seed)
    masks = np.zeros((len(centers), cap), dtype=np.uint8)
    for s, ci in enumerate(centers):
        cnt = len(column(o, ci))
        if cnt > npts:
            masks[s, rs.permutation(cnt)[:npts]] = 1
    return masks


def _scene_attrs(rs, n):
    return rs.randint(0, 9, n).astype(np.int32), rs.randint(0, 256, (n, 3)) / 255.0


def find_point(o, xyz):
    return int(np.flatnonzero((o.points == np.asarray(xyz, dtype=np.float64)).all(axis=1))[0])


# ---- B1: column faces -------------------------------------------------------------------------------------------------
LATTICE_NPTS = 512
LATTICE_CENTERS = ((10.0, 10.0, 0.0), (15.0, 7.5, 2.0), (12.5, 10.0, 1.0))  # z at the scene's floor, at its top, between


def lattice_scene():
    """every coordinate a multiple of 0.5 (exact): x 0 .. 30, y 0 .. 20, z 0 .. 2, 205 points per x value, shuffled"""
    rs = np.random.RandomState(110)
    g = np.stack(np.meshgrid(np.arange(61) * 0.5, np.arange(41) * 0.5, np.arange(5) * 0.5, indexing="ij"), -1).reshape(-1, 3)
    pts = g[rs.permutation(len(g))]
    labels, cols = _scene_attrs(rs, len(pts))
    return pts, labels, cols


# ---- B2: ends of the scene --------------------------------------------------------------------------------------------
ENDS_N, ENDS_NPTS = 700, 64


def ends_scene():
    rs = np.random.RandomState(120)
    pts = np.stack((rs.uniform(0, 30, ENDS_N), rs.uniform(0, 8, ENDS_N), rs.uniform(0, 3, ENDS_N)), 1)
    labels, cols = _scene_attrs(rs, ENDS_N)
    return pts, labels, cols


# ---- B3 / B4: columns of a chosen size --------------------------------------------------------------------------------
BLOCK_PITCH = 100.0


def block_scene(sizes, seed, split_y=False):
    """block k: sizes[k] points with x in [100 k, 100 k + 4], far from every other block, so the x-slab of a column around any
    of its points is exactly the block.  split_y: half of each block lies at y in [20, 24], outside every column around the
    other half (y in [0, 4]); otherwise the whole block is the column.  Rows shuffled."""
    rs = np.random.RandomState(seed)
    parts = []
    for k, size in enumerate(sizes):
        y = rs.uniform(0, 4, size)
        if split_y:
            y[rs.permutation(size)[:size // 2]] += 20.0
        parts.append(np.stack((BLOCK_PITCH * k + rs.uniform(0, 4, size), y, rs.uniform(0, 3, size)), 1))
    pts = np.concatenate(parts)
    pts = pts[rs.permutation(len(pts))]
    labels, cols = _scene_attrs(rs, len(pts))
    return pts, labels, cols


def block_center(o, k):
    """sorted index of the first point of block k with y < 10"""
    x, y = o.points[:, 0], o.points[:, 1]
    return int(np.flatnonzero((x >= BLOCK_PITCH * k) & (x < BLOCK_PITCH * k + 5) & (y < 10))[0])


CHUNK_SLABS = (1023, 1024, 1025, 3000)  # rows of the x-slab against the 1024 threads of the workgroup
CHUNK_NPTS = 256


def chunk_scene():
    return block_scene(CHUNK_SLABS, 130, split_y=True)


COUNT_NPTS = (5, 1024, 1500)


def count_sizes(npts):
    """cnt of the six columns: 1, 2, npts - 1, npts, npts + 1, 3 npts + 7"""
    return (1, 2, npts - 1, npts, npts + 1, 3 * npts + 7)


def count_scene(npts):
    return block_scene(count_sizes(npts), 140 + npts)


def count_plan(o, npts):
    """-> centres (8,), masks (8, cap), cap: the six columns, the npts + 1 one three times -- its mask drops the first, a middle
    and the last row --, the widest with a seeded random mask"""
    sizes = count_sizes(npts)
    blocks = [0, 1, 2, 3, 4, 4, 4, 5]
    centers = [block_center(o, k) for k in blocks]
    cap = max(sizes)
    masks = random_masks(o, centers, npts, cap, 150 + npts)
    for s, drop in zip((4, 5, 6), (0, (npts + 1) // 2, npts)):
        masks[s] = 0
        masks[s, :npts + 1] = 1
        masks[s, drop] = 0
    return np.array(centers), masks, cap


# ---- B8: far from the origin ------------------------------------------------------------------------------------------
FAR_OFFSET = (1.0e5, -2.0e5, 3.0e3)
FAR_NPTS = 256


def far_scene():
    rs = np.random.RandomState(180)
    n = 3000
    pts = np.stack((rs.uniform(0, 12, n), rs.uniform(0, 12, n), rs.uniform(0, 3, n)), 1) + np.array(FAR_OFFSET)
    labels, cols = _scene_attrs(rs, n)
    return pts, labels, cols


FAR_CENTERS = (5, 1500, 2990)
