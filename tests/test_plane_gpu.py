"""GPU tests of plane segmentation: pn2_plane_score / pn2_plane_ransac (csrc/pn2_plane.hip) against the numpy model of the rules
(tests/plane_ref.py) or against answers known by construction; every output between poisoned guards, every input compared
unchanged; pn2.plane's wrappers, the KITTI methods and the two examples.

There is no tolerance anywhere but in Plane.distance (stated there): the decisions are float64 comparisons in a fixed order
without contraction and everything after them is integer, so counts, headers, masks, sample indices and plane bits are compared
for equality.  Nothing here captures a graph."""
import ctypes
import importlib.util
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_ref as C  # noqa: E402
import plane_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64  # guard bytes in front of and behind every output
CHUNK = 1024  # kChunk of csrc/pn2_plane.hip: the points a workgroup of the scoring kernel stages per pass
SCORE_N = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 70001)
SCORE_PLANES = (1, 63, 64, 65, 255, 256, 257, 1000)


def _guarded(torch, dev, nbytes):
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _workspace(torch, pn2, dev, n, trials):
    nbytes = ctypes.c_ulonglong(0)
    pn2._lib.launch("pn2_plane_workspace_size", dev, n, trials, ctypes.byref(nbytes), stream=False)
    ws = torch.full((int(nbytes.value) + 255 + G,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    return ws, ws.data_ptr() + off, int(nbytes.value), off


def _score(pn2, dev, pts, planes, thr, labels=None):
    """pn2_plane_score -> counts (T,) int32, checked to stay inside its guards, the inputs unchanged"""
    import torch
    lib = pn2._lib
    planes = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 6)
    d_pts, d_pl = torch.from_numpy(pts).to(dev), torch.from_numpy(planes).to(dev)
    d_lab = None if labels is None else torch.from_numpy(labels).to(dev)
    raw, counts = _guarded(torch, dev, 4 * len(planes))
    lib.launch("pn2_plane_score", dev, len(pts), lib.ptr(d_pts), lib.ptr(d_lab), len(planes), lib.ptr(d_pl), float(thr),
               lib.ptr(counts))
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes(), "points changed"
    assert d_pl.cpu().numpy().tobytes() == planes.tobytes(), "planes changed"
    assert labels is None or d_lab.cpu().numpy().tobytes() == labels.tobytes(), "labels changed"
    return _payload(raw, 4 * len(planes), "counts").view(np.int32)


def _ransac(pn2, dev, pts, thr, trials, seed=0, labels=None, axis=None, cos2=0.0):
    """pn2_plane_ransac -> inlier (n,) uint8, plane (4,) float64, header (8,) int32: each inside its guards, the workspace not
    written past its size, the inputs unchanged"""
    import torch
    lib = pn2._lib
    n = len(pts)
    d_pts = torch.from_numpy(pts).to(dev)
    d_lab = None if labels is None else torch.from_numpy(labels).to(dev)
    raw_in, inlier = _guarded(torch, dev, n)
    raw_pl, plane = _guarded(torch, dev, 32)
    raw_hdr, hdr = _guarded(torch, dev, 32)
    ws, ws_ptr, ws_bytes, off = _workspace(torch, pn2, dev, n, trials)
    c_axis = None if axis is None else (ctypes.c_double * 3)(*axis)
    lib.launch("pn2_plane_ransac", dev, n, lib.ptr(d_pts), lib.ptr(d_lab), float(thr), trials, seed, c_axis, float(cos2),
               lib.ptr(inlier), lib.ptr(plane), lib.ptr(hdr), ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes(), "points changed"
    assert labels is None or d_lab.cpu().numpy().tobytes() == labels.tobytes(), "labels changed"
    h_ws = ws.cpu().numpy()
    assert (h_ws[:off] == POISON).all() and (h_ws[off + ws_bytes:] == POISON).all(), "workspace: written outside its bounds"
    return (_payload(raw_in, n, "inlier").copy(), _payload(raw_pl, 32, "plane").view(np.float64).copy(),
            _payload(raw_hdr, 32, "header").view(np.int32).copy())


def _check(pn2, dev, pts, thr, trials, seed=0, labels=None, axis=None, cos2=0.0):
    """the whole result against the model -> mask, plane, header"""
    mask, plane, hdr = _ransac(pn2, dev, pts, thr, trials, seed, labels, axis, cos2)
    want_mask, want_plane, want_hdr = R.ransac(pts, thr, trials, seed, labels, axis, cos2)
    assert hdr.tolist() == want_hdr.tolist(), "header"
    assert plane.tobytes() == want_plane.tobytes(), "plane bits: %r != %r" % (plane.tolist(), want_plane.tolist())
    assert np.array_equal(mask, want_mask), "%d mask entries differ" % (mask != want_mask).sum()
    assert int(mask.sum()) == hdr[1]
    return mask, plane, hdr


def _cloud(seed, n, bad=True):
    """n points: two thirds near the plane z = 0.1 x - 0.2 y + 1 (noise 0.02), the rest anywhere in a box; with `bad` a few
    non-finite rows and labels with some -1 -> points, labels"""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-8, 8, (n, 2))
    z = np.where(rs.random_sample(n) < 0.67, 0.1 * xy[:, 0] - 0.2 * xy[:, 1] + 1.0 + rs.normal(0, 0.02, n), rs.uniform(-3, 5, n))
    pts = np.column_stack([xy, z]).astype(np.float32)
    labels = rs.randint(0, 4, n).astype(np.int32)
    if bad and n > 8:
        pts[n // 3, 1], pts[n // 2, 0], pts[n - 2, 2] = np.nan, np.inf, -np.inf
        labels[rs.randint(0, n, n // 7 + 1)] = -1
    return pts, labels


def _planes_through(pts, count, seed):
    """`count` planes (count,6) through three random rows of pts each, every 17th void in one of four ways"""
    rs = np.random.RandomState(seed)
    P = pts.astype(np.float64)
    s = rs.randint(0, len(pts), (count, 3))
    with np.errstate(all="ignore"):
        planes = np.concatenate([P[s[:, 0]], np.cross(P[s[:, 1]] - P[s[:, 0]], P[s[:, 2]] - P[s[:, 0]])], 1)
    planes[~np.isfinite(planes).all(axis=1)] = [0, 0, 0, 0, 0, 1.0]  # a sample hit a non-finite row: the plane z = 0 instead
    planes[0] = [0, 0, 1.0, -0.1, 0.2, 1.0]  # the planted plane itself
    for k, void in zip(range(5, count, 17), [[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [1e200, 1, 1]] * count):
        planes[k, 3:] = void
    return planes


# ---- pn2_plane_score: sizes around wave, workgroup and chunk edges ---------------------------------------------------------------
@pytest.fixture(scope="module")
def score_case():
    """one cloud of the largest n and the most planes, the model's counts for every n of SCORE_N: counts[n][t]"""
    pts, labels = _cloud(21, max(SCORE_N))
    planes = _planes_through(pts[:60], max(SCORE_PLANES), 22)
    ok = R.valid_mask(pts, labels)
    table = np.zeros((len(SCORE_N), len(planes)), dtype=np.int32)
    for t, plane in enumerate(planes):
        run = np.cumsum(R.inliers(pts, plane, 0.05) & ok)
        table[:, t] = run[np.array(SCORE_N) - 1]
    assert table[-1].max() > 30000 and (table[-1] == 0).sum() >= 50 and len(np.unique(table[-1])) > 100
    frozen = pts.copy(), labels.copy(), planes.copy()
    return pts, labels, planes, dict(zip(SCORE_N, table)), frozen


@pytest.mark.parametrize("nplanes", SCORE_PLANES)
@pytest.mark.parametrize("n", SCORE_N)
def test_score_sizes(pn2, cuda, score_case, n, nplanes):
    pts, labels, planes, want, frozen = score_case
    got = _score(pn2, cuda, np.ascontiguousarray(pts[:n]), planes[:nplanes], 0.05, np.ascontiguousarray(labels[:n]))
    assert np.array_equal(got, want[n][:nplanes]), "%d counts differ" % (got != want[n][:nplanes]).sum()
    for a, b in zip((pts, labels, planes), frozen):
        assert a.tobytes() == b.tobytes(), "the shared case changed"


# ---- more chunks than chunk walkers: a workgroup goes through its chunk loop several times --------------------------------------
SCORE_BLOCKS = 2048  # kScoreBlocks of csrc/pn2_plane.hip: the grid is gx = ceil(planes / 256) by gy = min(chunks, ceil(2048 / gx))


def _chunk_walk(n, nplanes):
    """-> the chunks of n points, and gy: workgroup y stages the chunks y, y + gy, y + 2 gy, ..."""
    gx, chunks = -(-nplanes // 256), -(-n // CHUNK)
    return chunks, min(chunks, -(-SCORE_BLOCKS // gx))


@pytest.mark.parametrize("n,nplanes,passes,short_last", [
    (70001, 16384, 3, True),             # 69 chunks over 32 walkers: two or three passes, the short chunk as a third
    (5 * CHUNK + 17, 262144, 3, True),   # 6 chunks over 2 walkers: three passes each, the one of 17 points after two full ones
    (4 * CHUNK, 262144, 2, False),       # 4 full chunks over 2 walkers
    (2 * CHUNK + 1, 2 ** 19 + 3, 3, True)])  # 3 chunks, one walker: every workgroup stages all of them, the last of one point
def test_score_several_passes_through_the_chunk_loop(pn2, cuda, score_case, n, nplanes, passes, short_last):
    """The counts of one workgroup over several chunks: the stride of the walk, the barrier that guards the reuse of the stage,
    a short chunk staged over a full one.  The planes are the 1000 of the size cases repeated (the model scores each once)."""
    pts, labels, planes, want, frozen = score_case
    chunks, gy = _chunk_walk(n, nplanes)
    assert chunks > gy and -(-chunks // gy) == passes and (n % CHUNK != 0) == short_last
    many = np.resize(planes, (nplanes, 6))
    cut_pts, cut_lab = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(labels[:n])
    expect = want[n] if n in want else R.score(cut_pts, planes, 0.05, cut_lab)
    got = _score(pn2, cuda, cut_pts, many, 0.05, cut_lab)
    assert np.array_equal(got, np.resize(expect, nplanes)), "%d counts differ" % (got != np.resize(expect, nplanes)).sum()
    assert expect.max() > n // 3  # every chunk has points that count
    for a, b in zip((pts, labels, planes), frozen):
        assert a.tobytes() == b.tobytes(), "the shared case changed"


def few_valid_points(n, valid):
    """the cloud of _cloud with every label -1 but `valid` of them, spread from the first chunk to the last point: many trials
    over few valid points repeat their planes, so the model scores a few thousand planes for 2^18 trials"""
    pts, _ = _cloud(43, n, bad=False)
    labels = np.full(n, -1, dtype=np.int32)
    labels[np.linspace(3, n - 1, valid).astype(np.int64)] = 2
    return pts, labels


@pytest.mark.parametrize("seed", [0, 6])
def test_ransac_several_passes_through_the_chunk_loop(pn2, cuda, seed):
    n, trials = 5 * CHUNK + 17, 262144
    chunks, gy = _chunk_walk(n, trials)
    assert (chunks, gy) == (6, 2)
    pts, labels = few_valid_points(n, 20)
    mask, plane, hdr = _check(pn2, cuda, pts, 0.05, trials, seed, labels)
    at = np.nonzero(mask)[0]
    assert hdr[0] == 0 and hdr[6] == 20 and hdr[1] >= 8 and at[0] < CHUNK and at[-1] >= 4 * CHUNK  # inliers in far-apart chunks
    assert hdr[7] < trials * (20 * 19 * 18) / 20 ** 3 * 1.02  # repeated ranks are void: about 85 % of the trials are not


def test_score_without_labels_and_against_the_model_directly(pn2, cuda):
    pts, labels = _cloud(23, 3000)
    planes = _planes_through(pts, 300, 24)
    for lab in (None, labels):
        for thr in (0.05, 0.5, 1e-6):
            assert np.array_equal(_score(pn2, cuda, pts, planes, thr, lab), R.score(pts, planes, thr, lab))


# ---- the threshold -----------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive_and_exact(pn2, cuda):
    above = np.nextafter(np.float32(0.5), np.float32(1))
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 4, 0.5], [3, 4, above], [5, 5, -0.5], [-2, 7, -above], [6, 1, 0.25]],
                   dtype=np.float32)
    want = [True, True, True, True, False, True, False, True]
    # the plane z = 0 through integer points; then normals that are not of unit length: e and nn scale together, exactly for
    # powers of two and to the last bit of the fixed formula otherwise (the model decides, the expected answer is the same)
    planes = np.array([[7, -2, 0, 0, 0, s] for s in (1.0, 2.0, 3.0, 0.7, 1e-3, 1e150, -5.0)], dtype=np.float64)
    counts = _score(pn2, cuda, pts, planes, 0.5)
    assert counts.tolist() == [sum(want)] * len(planes) == R.score(pts, planes, 0.5).tolist()
    for k in range(len(pts)):  # point by point
        assert _score(pn2, cuda, pts[k:k + 1].copy(), planes, 0.5).tolist() == [int(want[k])] * len(planes), k
    # through pn2_plane_ransac: 36 integer points of z = 0 and one point above them
    grid = np.stack(np.meshgrid(np.arange(6), np.arange(6)), -1).reshape(-1, 2)
    for extra, inside in (([3, 4, 0.5], 1), ([3, 4, above], 0)):
        cloud = np.concatenate([np.column_stack([grid, np.zeros(36)]), [extra]]).astype(np.float32)
        mask, plane, hdr = _check(pn2, cuda, cloud, 0.5, 65, 3)
        assert hdr[0] == 0 and mask[:36].all() and mask[36] == inside and hdr[1] == 36 + inside


# ---- void planes ---------------------------------------------------------------------------------------------------------------
def test_void_planes_score_zero_and_leave_their_neighbours_alone(pn2, cuda):
    pts, _ = _cloud(25, 2000, bad=False)
    good = np.array([0, 0, 1.0, -0.1, 0.2, 1.0])
    voids = [[0, 0, 1, 0, 0, 0], [0, 0, 1, np.nan, 0.2, 1], [0, 0, 1, -0.1, np.inf, 1], [0, 0, 1, -np.inf, 0, 0], [0, 0, 1, 1e200, 0.2, 1],
             [0, 0, 1, 1e-170, 1e-170, 1e-170]]  # the last: nn underflows to 0
    planes = np.array([good if k % 2 == 0 else voids[(k // 2) % len(voids)] for k in range(130)], dtype=np.float64)
    counts = _score(pn2, cuda, pts, planes, 0.05)
    full = int(R.score(pts, good[None], 0.05)[0])
    assert full > 1000 and counts[0::2].tolist() == [full] * 65 and counts[1::2].tolist() == [0] * 65
    assert np.array_equal(counts, R.score(pts, planes, 0.05))
    # a non-finite origin under a finite normal is no void plane by the rule, but nothing is within reach of it
    odd = np.array([[np.nan, 0, 1, -0.1, 0.2, 1], [0, np.inf, 1, -0.1, 0.2, 1], good], dtype=np.float64)
    assert _score(pn2, cuda, pts, odd, 0.05).tolist() == [0, 0, full] == R.score(pts, odd, 0.05).tolist()


# ---- invalid points ------------------------------------------------------------------------------------------------------------
def test_invalid_points_are_not_counted(pn2, cuda):
    pts, _ = _cloud(26, 1500, bad=False)
    plane = np.array([[0, 0, 1.0, -0.1, 0.2, 1.0]])
    clean = _score(pn2, cuda, pts, plane, 0.05)[0]
    on = np.nonzero(R.inliers(pts, plane[0], 0.05))[0]
    bad = pts.copy()
    bad[on[0], 0], bad[on[1], 1], bad[on[2], 2], bad[on[3]] = np.nan, np.inf, -np.inf, np.nan
    assert _score(pn2, cuda, bad, plane, 0.05)[0] == clean - 4
    labels = np.zeros(len(pts), dtype=np.int32)
    labels[on[4:10]] = [-1, -7, -2 ** 31, -1, -1, -3]
    assert _score(pn2, cuda, bad, plane, 0.05, labels)[0] == clean - 10
    mask, _, hdr = _check(pn2, cuda, bad, 0.05, 65, 1, labels)
    assert hdr[0] == 0 and not mask[on[:10]].any() and hdr[6] == len(pts) - 10
    # coordinates of 1e30 next to ordinary ones: finite, valid, far away -- and no NaN that would miscount
    far = pts.copy()
    far[on[0]], far[on[1], 2], far[5] = 1e30, -1e30, [1e30, 1e30, 3e38]
    planes = _planes_through(far[:200], 64, 27)
    assert np.array_equal(_score(pn2, cuda, far, planes, 0.05), R.score(far, planes, 0.05))
    assert _score(pn2, cuda, far, plane, 0.05)[0] == R.score(far, plane, 0.05)[0] <= clean - 2
    _check(pn2, cuda, far, 0.05, 65, 2)


# ---- pn2_plane_ransac against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 5, 2 ** 63 + 11])
@pytest.mark.parametrize("trials", [1, 65, 257])
@pytest.mark.parametrize("n", [3, 4, 65, 1025, 70001])
def test_ransac_against_the_model(pn2, cuda, n, trials, seed):
    pts, labels = _cloud(30 + n % 7, n, bad=n > 8)
    mask, plane, hdr = _check(pn2, cuda, pts, 0.05, trials, seed, labels)
    V = int(R.valid_mask(pts, labels).sum())
    assert hdr[6] == V and (n < 65 or V & (V - 1) != 0)  # not a power of two: the modulo is no mask
    if hdr[0] == 0:
        assert mask[hdr[3]] == 1 and hdr[7] >= 1 and 0 <= hdr[2] < trials
    _check(pn2, cuda, pts, 0.05, trials, seed)  # without labels


def test_more_blocks_than_one_pass_of_the_block_scan(pn2, cuda):
    """256 * 256 + 300 points: the counts of the compaction's blocks no longer fit one pass of the one-workgroup scan"""
    n = 256 * 256 + 300
    pts, labels = _cloud(41, n)
    mask, plane, hdr = _check(pn2, cuda, pts, 0.05, 33, 9, labels)
    assert hdr[0] == 0 and max(hdr[3:6]) > 256 * 128  # samples from all over the cloud


def test_planted_ground(pn2, cuda):
    """the case pinned in tests/test_plane_cpu.py (plane_ref.planted): 1800 of 3000 points a ground of slope 0.02, noise 0.03, thr 0.05, 64 trials"""
    pts = R.planted()
    mask, plane, hdr = _check(pn2, cuda, pts, 0.05, 64, 7)
    assert hdr.tolist() == [0, 1539, 14, 1377, 530, 619, 3000, 64]


# ---- ties ----------------------------------------------------------------------------------------------------------------------
def tie_cloud():
    """two parallel sheets z = 0 and z = 1 of 400 integer points each, interleaved: every plane through three points of one sheet
    that are not collinear holds exactly that sheet (integer arithmetic, nothing rounds), so many trials tie at 400"""
    rs = np.random.RandomState(50)
    xy = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2)
    sheets = np.concatenate([np.column_stack([xy, np.zeros(400)]), np.column_stack([xy, np.ones(400)])])
    return np.ascontiguousarray(sheets[rs.permutation(800)].astype(np.float32))


def test_tie_goes_to_the_lowest_trial(pn2, cuda):
    pts = tie_cloud()
    trials, seed = 65, 4
    planes, sample, live = R.hypotheses(pts, np.arange(800), seed, trials)
    counts = R.score(pts, planes, 0.25)
    winners = np.nonzero(counts == counts.max())[0]
    assert counts.max() == 400 and len(winners) >= 4
    assert len({float(pts[sample[t, 0], 2]) for t in winners}) == 2  # planes of both sheets among them
    mask, plane, hdr = _check(pn2, cuda, pts, 0.25, trials, seed)
    assert hdr[2] == winners[0] and hdr[1] == 400 and winners[0] > 0
    assert np.array_equal(mask.astype(bool), pts[:, 2] == pts[sample[winners[0], 0], 2])


# ---- the axis constraint and the orientation -------------------------------------------------------------------------------------
def wall_and_ground():
    """a wall x = 5 of 2000 points and a ground z = 0 of 1000, exact coordinates in the plane's own axis, shuffled"""
    rs = np.random.RandomState(60)
    wall = np.column_stack([np.full(2000, 5.0), rs.uniform(-10, 10, 2000), rs.uniform(0, 6, 2000)])
    ground = np.column_stack([rs.uniform(-10, 10, 1000), rs.uniform(-10, 10, 1000), np.zeros(1000)])
    return np.ascontiguousarray(np.concatenate([wall, ground])[rs.permutation(3000)].astype(np.float32))


def test_axis_constraint_and_orientation(pn2, cuda):
    pts = wall_and_ground()
    on_wall, on_ground = pts[:, 0] == 5.0, pts[:, 2] == 0.0
    trials, seed, cos2 = 257, 1, R.cos2_of(15.0)
    mask, plane, hdr = _check(pn2, cuda, pts, 0.05, trials, seed)
    assert hdr[1] >= 2000 and mask[on_wall].all()  # without an axis the wall wins
    assert plane[2] == 0 and plane[1] == 0 and plane[0] > 0  # the first non-zero of (c,b,a) is positive
    up = _check(pn2, cuda, pts, 0.05, trials, seed, axis=(0.0, 0.0, 1.0), cos2=cos2)
    assert 1000 <= up[2][1] < 2000 and up[0][on_ground].all() and up[2][7] < hdr[7]  # the ground; fewer trials are non-void
    assert up[1][2] > 0 and up[1][0] == 0 and up[1][1] == 0
    down = _check(pn2, cuda, pts, 0.05, trials, seed, axis=(0.0, 0.0, -2.0), cos2=cos2)  # the axis's length does not matter
    assert np.array_equal(down[0], up[0]) and down[2].tolist() == up[2].tolist()
    assert down[1].tobytes() == (-up[1]).tobytes()  # the same plane, negated exactly: dt >= 0
    # an axis along the wall's normal, and a cone so narrow that every trial is void: status 2
    along = _check(pn2, cuda, pts, 0.05, trials, seed, axis=(-1.0, 0.0, 0.0), cos2=cos2)
    assert along[2][1] >= 2000 and along[1][0] < 0
    none = _check(pn2, cuda, pts, 0.05, trials, seed, axis=(1.0, 1.0, 1.0), cos2=R.cos2_of(1.0))
    assert none[2].tolist() == [2, 0, 0, -1, -1, -1, 3000, 0]
    # cos2 = 0 excludes nothing, cos2 = 1 only exact alignment
    assert _check(pn2, cuda, pts, 0.05, trials, seed, axis=(0.0, 1.0, 0.0), cos2=0.0)[2][7] == hdr[7]
    _check(pn2, cuda, pts, 0.05, trials, seed, axis=(0.0, 0.0, 1.0), cos2=1.0)


def test_orientation_without_axis(pn2, cuda):
    rs = np.random.RandomState(61)
    flat = np.column_stack([rs.uniform(-5, 5, (500, 2)), np.zeros(500)])
    for perm, sign_at in (((0, 1, 2), 2), ((0, 2, 1), 1), ((2, 0, 1), 0)):  # the plane's normal along z, y, x
        pts = np.ascontiguousarray(flat[:, perm].astype(np.float32))
        for seed in range(4):  # the cross product comes out with either sign
            _, plane, hdr = _check(pn2, cuda, pts, 0.01, 1, seed)
            if hdr[0] == 0:
                assert plane[sign_at] > 0 and hdr[1] == 500
    pts, _ = _cloud(62, 500, bad=False)
    for seed in range(6):
        _, plane, hdr = _check(pn2, cuda, pts, 0.05, 1, seed)
        assert hdr[0] != 0 or plane[2] > 0


# ---- statuses ------------------------------------------------------------------------------------------------------------------
def test_status_fewer_than_three_valid_points(pn2, cuda):
    none = [0, 0, -1, -1, -1]
    two = np.array([[0, 0, 0], [np.nan, 1, 1], [1, 1, 1], [2, np.inf, 0]], dtype=np.float32)
    mask, plane, hdr = _check(pn2, cuda, two, 0.1, 65)
    assert hdr.tolist() == [1] + none + [2, 0] and not mask.any() and plane.tobytes() == np.zeros(4).tobytes()
    labels = np.array([0, 0, -1, 0], dtype=np.int32)
    assert _check(pn2, cuda, two, 0.1, 65, 0, labels)[2].tolist() == [1] + none + [1, 0]
    nothing = np.full((70, 3), np.nan, dtype=np.float32)
    mask, plane, hdr = _check(pn2, cuda, nothing, 0.1, 257)
    assert hdr.tolist() == [1] + none + [0, 0] and not mask.any() and plane.tobytes() == np.zeros(4).tobytes()
    pts, _ = _cloud(70, 300, bad=False)
    assert _check(pn2, cuda, pts, 0.1, 8, 0, np.full(300, -1, dtype=np.int32))[2].tolist() == [1] + none + [0, 0]
    one = np.array([[1, 2, 3]], dtype=np.float32)
    assert _check(pn2, cuda, one, 0.1, 1)[2].tolist() == [1] + none + [1, 0]


def test_status_every_trial_void(pn2, cuda):
    line = np.outer(np.arange(300), [1.0, 2.0, -0.5]).astype(np.float32)  # exact: every cross product is zero
    mask, plane, hdr = _check(pn2, cuda, line, 0.1, 257, 3)
    assert hdr.tolist() == [2, 0, 0, -1, -1, -1, 300, 0] and not mask.any() and plane.tobytes() == np.zeros(4).tobytes()
    same = np.tile(np.array([[1.5, -2.25, 0.125]], dtype=np.float32), (100, 1))  # coincident points
    assert _check(pn2, cuda, same, 0.1, 65)[2].tolist() == [2, 0, 0, -1, -1, -1, 100, 0]
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)  # repeated ranks are void, distinct ones are not
    planes, _, live = R.hypotheses(three, np.arange(3), 0, 65)
    assert 0 < live.sum() < 65
    assert _check(pn2, cuda, three, 0.1, 65)[2][7] == live.sum()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pn2, cuda):
    import torch
    lib, K = pn2._lib, pn2._lib.ABI.constants
    n, trials = 100, 64
    d_pts = torch.zeros((n, 3), dtype=torch.float32, device=cuda)
    d_lab = torch.zeros((n,), dtype=torch.int32, device=cuda)
    d_planes = torch.ones((10, 6), dtype=torch.float64, device=cuda)
    raw_in, inlier = _guarded(torch, cuda, n)
    raw_pl, plane = _guarded(torch, cuda, 32)
    raw_hdr, hdr = _guarded(torch, cuda, 32)
    raw_cnt, counts = _guarded(torch, cuda, 40)
    ws, ws_ptr, ws_bytes, _ = _workspace(torch, pn2, cuda, n, trials)
    axis = lambda *v: (ctypes.c_double * 3)(*v)  # noqa: E731
    good = dict(n=n, points=lib.ptr(d_pts), labels=lib.ptr(d_lab), thr=0.5, trials=trials, seed=3, axis=None, cos2=0.0,
                inlier=lib.ptr(inlier), plane=lib.ptr(plane), header=lib.ptr(hdr), workspace=ws_ptr, workspace_bytes=ws_bytes,
                stream=lib.stream_ptr())
    names = lib.ABI.functions["pn2_plane_ransac"].argnames
    cases = [(dict(n=0), "EINVAL"), (dict(n=-1), "EINVAL"), (dict(trials=0), "EINVAL"), (dict(trials=2 ** 20 + 1), "EINVAL"),
             (dict(thr=0.0), "EINVAL"), (dict(thr=-0.5), "EINVAL"), (dict(thr=float("nan")), "EINVAL"),
             (dict(thr=float("inf")), "EINVAL"), (dict(axis=axis(0, 0, 1), cos2=1.25), "EINVAL"),
             (dict(axis=axis(0, 0, 1), cos2=float("nan")), "EINVAL"), (dict(axis=axis(0, 0, 0), cos2=0.5), "EINVAL"),
             (dict(axis=axis(0, float("inf"), 0), cos2=0.5), "EINVAL"), (dict(points=None), "ENULL"), (dict(inlier=None), "ENULL"),
             (dict(plane=None), "ENULL"), (dict(header=None), "ENULL"), (dict(workspace=None), "ENULL"),
             (dict(workspace_bytes=ws_bytes - 1), "EINVAL"), (dict(workspace_bytes=0), "EINVAL"),
             (dict(workspace=ws_ptr + 4), "EINVAL"), (dict(plane=ctypes.c_void_p(plane.data_ptr() + 4)), "EINVAL"),
             (dict(header=ctypes.c_void_p(hdr.data_ptr() + 2)), "EINVAL")]
    score_good = dict(n=n, points=lib.ptr(d_pts), labels=lib.ptr(d_lab), nplanes=10, planes=lib.ptr(d_planes), thr=0.5,
                      counts=lib.ptr(counts), stream=lib.stream_ptr())
    score_names = lib.ABI.functions["pn2_plane_score"].argnames
    score_cases = [(dict(n=0), "EINVAL"), (dict(nplanes=0), "EINVAL"), (dict(thr=0.0), "EINVAL"), (dict(thr=float("nan")), "EINVAL"),
                   (dict(points=None), "ENULL"), (dict(planes=None), "ENULL"), (dict(counts=None), "ENULL"),
                   (dict(planes=ctypes.c_void_p(d_planes.data_ptr() + 4)), "EINVAL"),
                   (dict(counts=ctypes.c_void_p(counts.data_ptr() + 2)), "EINVAL")]
    with torch.cuda.device(cuda):
        for change, code in cases:
            a = dict(good, **change)
            assert lib.lib.pn2_plane_ransac(*[a[k] for k in names]) == K["PN2_" + code], change
        for change, code in score_cases:
            a = dict(score_good, **change)
            assert lib.lib.pn2_plane_score(*[a[k] for k in score_names]) == K["PN2_" + code], change
    torch.cuda.synchronize()
    for raw, nbytes, what in ((raw_in, n, "inlier"), (raw_pl, 32, "plane"), (raw_hdr, 32, "header"), (raw_cnt, 40, "counts")):
        assert (_payload(raw, nbytes, what) == POISON).all(), what
    assert (ws.cpu().numpy() == POISON).all(), "the workspace was written"


# ---- the wrappers --------------------------------------------------------------------------------------------------------------
def _same_plane(torch, pn2, dev, got, want_mask, want_plane, want_hdr):
    assert isinstance(got, pn2.Plane) and got.status == want_hdr[0] and got.count == want_hdr[1] and got.trial == want_hdr[2]
    assert got.sample == tuple(want_hdr[3:6].tolist()) and got.valid == want_hdr[6]
    assert got.inliers.dtype == torch.bool and got.inliers.device == dev and np.array_equal(got.inliers.cpu().numpy(), want_mask != 0)
    assert got.raw.dtype == torch.float64 and got.raw.cpu().numpy().tobytes() == want_plane.tobytes()
    assert got.model.dtype == torch.float64 and got.model.device == dev and tuple(got.model.shape) == (4,)


def test_segment_plane_wrapper_and_distance(pn2, cuda):
    import torch
    pts64 = R.planted().astype(np.float64) * 1.0000001  # not float32 values: the wrapper casts
    labels64 = np.random.RandomState(80).randint(0, 6, 3000).astype(np.int64)
    pts32 = pts64.astype(np.float32)
    want = R.ransac(pts32, 0.05, 100, 7)
    assert want[2][0] == 0 and want[2][1] > 1400
    _same_plane(torch, pn2, cuda, pn2.segment_plane(pts64, 0.05, trials=100, seed=7), *want)  # numpy, float64
    d_pts, d_lab = torch.from_numpy(pts64).to(cuda), torch.from_numpy(labels64).to(cuda)
    plane = pn2.segment_plane(d_pts, 0.05, trials=100, seed=7)  # tensors
    _same_plane(torch, pn2, cuda, plane, *want)
    # classes: every other label counts as -1
    lab = np.where(np.isin(labels64, [1, 4]), labels64, -1).astype(np.int32)
    want_cls = R.ransac(pts32, 0.05, 100, 7, lab)
    for got in (pn2.segment_plane(d_pts, 0.05, trials=100, seed=7, labels=d_lab, classes=iter([4, 1, 1])),
                pn2.segment_plane(pts64, 0.05, trials=100, seed=7, labels=labels64, classes=(1, 4))):
        _same_plane(torch, pn2, cuda, got, *want_cls)
        assert got.valid == (lab >= 0).sum() and not got.inliers.cpu().numpy()[lab < 0].any()
    # the axis: max_angle in degrees becomes cos2 = cos(radians(max_angle)) ** 2, the double the model takes
    want_up = R.ransac(pts32, 0.05, 100, 7, None, (0.0, 0.0, 1.0), R.cos2_of(15.0))
    up = pn2.segment_plane(d_pts, 0.05, trials=100, seed=7, axis=(0, 0, 1), max_angle=15)
    _same_plane(torch, pn2, cuda, up, *want_up)
    assert up.model[2] > 0.99
    # model and distance: float64 numpy from the exact raw plane.  The ONE tolerance of this file: torch's sqrt and division are
    # taken as correctly rounded to within an ulp or two, so 4 ulp of float64 relative to the largest term of the sum
    raw = want[1]
    unit = raw / np.sqrt((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2])
    assert np.abs(plane.model.cpu().numpy() - unit).max() <= 4 * np.finfo(np.float64).eps * np.abs(unit).max()
    terms = np.column_stack([pts64 * unit[:3], np.full(3000, unit[3])])
    want_dist = ((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]
    bound = 4 * np.finfo(np.float64).eps * np.abs(terms).max(axis=1)
    for got in (plane.distance(d_pts), plane.distance(pts64)):
        assert got.dtype == torch.float64 and got.device == cuda
        err = np.abs(got.cpu().numpy() - want_dist)
        print("Plane.distance: largest error over its bound %.3g" % (err / bound).max())
        assert (err <= bound).all()
    assert (np.abs(want_dist[want[0] != 0]) <= 0.05 + 1e-5).all()  # the inliers, by the float64 points: within a hair of thr
    # no plane is an answer, and so is no point
    for bad, status, valid in ((pts64[:2], 1, 2), (np.outer(np.arange(40), [1.0, 1.0, 2.0]), 2, 40)):
        got = pn2.segment_plane(bad, 0.05, trials=30)
        assert (got.status, got.count, got.sample, got.trial, got.valid) == (status, 0, (-1, -1, -1), 0, valid)
        assert not got.inliers.any() and got.inliers.shape == (len(bad),) and (got.raw == 0).all() and (got.model == 0).all()
    empty = pn2.segment_plane(d_pts[:0], 0.05)
    assert empty.status == 1 and empty.count == 0 and empty.inliers.shape == (0,) and empty.valid == 0
    assert pn2.segment_planes(d_pts[:0], 0.05, 3, 10) == []


def three_planes():
    """3000 / 2000 / 1000 points on z = 0, x = 0, y = 0 (noise 0.005 across) in a 10 x 10 x 10 room, 400 of clutter; shuffled
    -> points, which (0, 1, 2, or 3 for clutter)"""
    rs = np.random.RandomState(90)
    sizes = [3000, 2000, 1000, 400]
    room = rs.uniform(0.5, 10, (sum(sizes), 3))
    which = np.repeat(np.arange(4), sizes)
    for k, axis in enumerate((2, 0, 1)):
        room[which == k, axis] = rs.normal(0, 0.005, sizes[k])
    order = rs.permutation(len(room))
    return np.ascontiguousarray(room[order].astype(np.float32)), which[order]


def test_segment_planes_peels_in_order_of_size(pn2, cuda):
    import torch
    pts, which = three_planes()
    # the model, peeled the same way
    labels = np.zeros(len(pts), dtype=np.int32)
    want = []
    for k in range(5):
        r = R.ransac(pts, 0.03, 200, 11 + k, labels)
        want.append(r)
        labels[r[0] != 0] = -1
    assert [w[2][1] >= 500 for w in want] == [True, True, True, False, False]
    planes = pn2.segment_planes(pts, 0.03, max_planes=5, min_inliers=500, trials=200, seed=11)
    assert len(planes) == 3  # it stops at the first plane below min_inliers, which is not returned
    for k, (got, w) in enumerate(zip(planes, want)):
        _same_plane(torch, pn2, cuda, got, *w)
        hit = got.inliers.cpu().numpy()
        assert hit[which == k].mean() > 0.99 and (which[hit] == k).mean() > 0.97 and abs(float(got.model[(2, 0, 1)[k]])) > 0.999
    assert [p.count for p in planes] == sorted((p.count for p in planes), reverse=True)
    taken = torch.stack([p.inliers for p in planes]).sum(0)
    assert int(taken.max()) == 1  # a point leaves the valid set with its plane
    assert [p.valid for p in planes] == [6400, 6400 - planes[0].count, 6400 - planes[0].count - planes[1].count]
    two = pn2.segment_planes(torch.from_numpy(pts).to(cuda), 0.03, 2, 500, trials=200, seed=11)  # max_planes stops it too
    assert len(two) == 2 and two[1].raw.cpu().numpy().tobytes() == want[1][1].tobytes()
    assert pn2.segment_planes(pts, 0.03, 5, 5000, trials=200, seed=11) == []
    # labels given: -1 stays out, and classes select
    lab = np.where(which == 0, -1, which).astype(np.int64)
    rest = pn2.segment_planes(pts, 0.03, 5, 500, trials=200, seed=11, labels=lab)
    assert len(rest) == 2 and all(not p.inliers.cpu().numpy()[which == 0].any() for p in rest)
    only = pn2.segment_planes(pts, 0.03, 5, 500, trials=200, seed=11, labels=which, classes=[1])
    assert len(only) == 1 and (which[only[0].inliers.cpu().numpy()] == 1).all()


def test_score_planes_wrapper(pn2, cuda):
    import torch
    pts, which = three_planes()
    planes6 = _planes_through(pts, 70, 91)
    want = R.score(pts, planes6, 0.03)
    got = pn2.score_planes(pts, planes6, 0.03)
    assert got.dtype == torch.int32 and got.device == cuda and np.array_equal(got.cpu().numpy(), want)
    d_pts = torch.from_numpy(pts).to(cuda)
    assert np.array_equal(pn2.score_planes(d_pts, torch.from_numpy(planes6).to(cuda), 0.03).cpu().numpy(), want)
    lab = np.where(which == 3, -1, which).astype(np.int64)
    assert np.array_equal(pn2.score_planes(d_pts, planes6, 0.03, labels=lab).cpu().numpy(), R.score(pts, planes6, 0.03, lab.astype(np.int32)))
    # (T,4) rows (a,b,c,d): the documented conversion, repeated here in numpy -- the origin is the plane's point nearest (0,0,0)
    found = pn2.segment_planes(d_pts, 0.03, 3, 500, trials=200, seed=11)
    rows = torch.stack([p.raw for p in found] + [p.model for p in found])
    h = rows.cpu().numpy()
    with np.errstate(all="ignore"):
        nn = (h[:, 0:1] * h[:, 0:1] + h[:, 1:2] * h[:, 1:2]) + h[:, 2:3] * h[:, 2:3]
        as6 = np.concatenate([h[:, :3] * (-h[:, 3:] / nn), h[:, :3]], 1)
    got4 = pn2.score_planes(d_pts, rows, 0.03).cpu().numpy()
    assert np.array_equal(got4, R.score(pts, as6, 0.03)) and np.array_equal(pn2.score_planes(pts, h, 0.03).cpu().numpy(), got4)
    assert got4[0] >= 2900 and got4[0] > got4[1] > got4[2] >= 900  # last frame's planes, scored on the whole cloud
    zero = pn2.score_planes(d_pts, np.zeros((3, 4)), 0.03)  # 0 / 0: a void plane, no error
    assert zero.tolist() == [0, 0, 0]
    assert pn2.score_planes(d_pts, np.zeros((0, 6)), 0.03).shape == (0,) and pn2.score_planes(d_pts[:0], planes6, 0.03).tolist() == [0] * 70


# ---- the KITTI methods -----------------------------------------------------------------------------------------------------------
def test_kitti_ground_and_objects(pn2, cuda):
    import torch
    rs = np.random.RandomState(95)
    n_ground, n_obj = 4000, 2500
    ground = np.column_stack([rs.uniform(-20, 20, (n_ground, 2)), rs.normal(0, 0.02, n_ground)])
    centre = rs.uniform(-18, 18, (25, 2))
    which = rs.randint(0, 25, n_obj)
    cars = np.column_stack([centre[which] + rs.uniform(0, 2, (n_obj, 2)), rs.uniform(0.0, 1.5, n_obj)])  # they stand on the ground
    order = rs.permutation(n_ground + n_obj)
    pts = np.ascontiguousarray(np.concatenate([ground, cars])[order].astype(np.float32))
    labels = np.concatenate([np.ones(n_ground), np.full(n_obj, 8)])[order].astype(np.int32)
    labels[rs.randint(0, len(labels), 300)] = 8  # the network calls some of the ground "car": they bridge the cars
    d_pts, d_lab = torch.from_numpy(pts).to(cuda), torch.from_numpy(labels).to(cuda)
    frame = types.SimpleNamespace(points=d_pts)
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)  # the methods use none of the network's state
    plane = predictor.ground_for_frame(frame, 0.1, trials=128, seed=2)
    want = R.ransac(pts, 0.1, 128, 2, None, (0.0, 0.0, 1.0), R.cos2_of(15.0))
    _same_plane(torch, pn2, cuda, plane, *want)
    assert plane.count > 3900 and plane.model[2] > 0.999
    with_labels = predictor.ground_for_frame(frame, 0.1, trials=128, seed=2, max_angle=10.0, dense_labels=d_lab, classes=[1])
    _same_plane(torch, pn2, cuda, with_labels, *R.ransac(pts, 0.1, 128, 2, np.where(labels == 1, 1, -1).astype(np.int32),
                                                        (0.0, 0.0, 1.0), R.cos2_of(10.0)))
    # objects without the ground == the clustering of the same cloud with those labels set to -1
    got = predictor.objects_for_frame(frame, d_lab, 0.5, [8], min_points=5, exclude=plane.inliers)
    cut = np.where(want[0] != 0, -1, np.where(labels == 8, 8, -1)).astype(np.int32)
    want_ids, want_hdr = C.cluster(pts, 0.5, cut, 5, 0)
    assert got.count == want_hdr[1] and np.array_equal(got.ids.cpu().numpy(), want_ids)
    direct = pn2.euclidean_clusters(d_pts, 0.5, labels=torch.from_numpy(cut).to(cuda), min_points=5)
    assert direct.count == got.count and torch.equal(direct.ids, got.ids) and torch.equal(direct.bbox, got.bbox)
    assert np.array_equal(predictor.objects_for_frame(frame, labels, 0.5, [8], min_points=5,
                                                      exclude=plane.inliers.cpu().numpy()).ids.cpu().numpy(), want_ids)
    # exclude=None is the old call
    old = predictor.objects_for_frame(frame, d_lab, 0.5, [8], min_points=5)
    new = predictor.objects_for_frame(frame, d_lab, 0.5, [8], min_points=5, exclude=None)
    plain = pn2.euclidean_clusters(d_pts, 0.5, labels=d_lab, classes=[8], min_points=5)
    for other in (new, plain):
        assert old.count == other.count
        for a, b in zip(old, other):
            assert a == b if isinstance(a, int) else torch.equal(a, b)
    assert not torch.equal(got.ids, old.ids)  # the ground took the cars' lowest points
    with pytest.raises(ValueError, match="exclude"):
        predictor.objects_for_frame(frame, d_lab, 0.5, [8], exclude=plane.inliers[:10])


# ---- the examples --------------------------------------------------------------------------------------------------------------
def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _png_size(path):
    with open(path, "rb") as f:
        png = f.read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", png[16:24])


def test_segment_planes_example_on_a_synthetic_scene(pn2, cuda, tmp_path):
    n = 6000
    out = str(tmp_path / "planes")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "segment_planes.py"), "--synthetic", str(n), "--out", out,
                          "--max_planes", "5", "--min_inliers", "300", "--trials", "256", "--seed", "3", "--width", "320",
                          "--height", "200"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    example = _example("segment_planes")
    pts = example.synthetic(n)
    labels = np.zeros(n, dtype=np.int32)
    want = []
    for k in range(5):
        mask, plane, hdr = R.ransac(pts, example.SYNTHETIC_THRESHOLD, 256, 3 + k, labels)
        if hdr[1] < 300:
            break
        want.append("%d %d %s" % (k, hdr[1], " ".join(repr(float(v)) for v in plane)))
        labels[mask != 0] = -1
    assert len(want) == 3
    with open(os.path.join(out, "planes.txt")) as f:
        assert f.read().splitlines() == want
    assert "3 planes, %d of %d points on one" % ((labels < 0).sum(), n) in run.stdout
    assert _png_size(os.path.join(out, "planes.png")) == (320, 200)


def test_cluster_objects_example_with_ground(pn2, cuda, tmp_path):
    n = 3000
    out = str(tmp_path / "objects")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_objects.py"), "--synthetic", str(n), "--out", out,
                          "--min_points", "5", "--ground", "0.01", "--ground-trials", "128", "--width", "320", "--height", "200"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    example = _example("cluster_objects")
    pts, labels = example.synthetic(n)  # its blobs lie around z = 0: a thin "ground" takes a slice out of every one
    mask, plane, hdr = R.ransac(pts, 0.01, 128, 0, None, (0.0, 0.0, 1.0), R.cos2_of(example.GROUND_MAX_ANGLE))
    assert hdr[0] == 0 and 300 < hdr[1] < 1500
    cut = np.where(mask != 0, -1, labels).astype(np.int32)
    ids, chdr = C.cluster(pts, example.SYNTHETIC_EPS, cut, 5, 0)
    first, size, label, bbox = C.stats(pts, ids, cut, int(chdr[1]))
    want = ["ground %d %s" % (hdr[1], " ".join(repr(float(v)) for v in plane))]
    want += ["%d %d %d %s" % (c, label[c], size[c], " ".join(repr(float(v)) for v in bbox[c])) for c in range(chdr[1])]
    with open(os.path.join(out, "objects.txt")) as f:
        assert f.read().splitlines() == want
    assert "ground: %d of %d points" % (hdr[1], n) in run.stdout and int(size.sum()) <= n - hdr[1]
    assert _png_size(os.path.join(out, "objects.png")) == (320, 200)
