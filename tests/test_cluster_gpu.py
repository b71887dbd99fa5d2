"""GPU tests of Euclidean clustering: pn2_cluster_points / pn2_cluster_stats / pn2_cluster_colors (csrc/pn2_cluster.hip) against the
numpy model of the rules (tests/cluster_ref.py) or, beyond the model's reach, against answers known by construction; every output
between poisoned guards, every input compared unchanged; pn2.cluster's wrapper, the KITTI method and examples/cluster_objects.py.

There is no tolerance anywhere: the link test is float64 in a fixed association without contraction and everything after it is
integer, so ids, headers, sizes, firsts, labels, box bits and colours are compared for equality.  Nothing here captures a graph."""
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

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64  # guard bytes in front of and behind every output
BLOCK = 256  # threads per workgroup and points per scan block; the block counts are scanned BLOCK at a time by one workgroup


def _guarded(torch, dev, nbytes):
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _workspace(torch, pn2, dev, n):
    nbytes = ctypes.c_ulonglong(0)
    pn2._lib.launch("pn2_cluster_workspace_size", dev, n, ctypes.byref(nbytes), stream=False)
    ws = torch.full((int(nbytes.value) + 255,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    return ws, ws.data_ptr() + off, ws.numel() - off


def _cluster(pn2, dev, pts, eps, labels=None, min_points=1, max_points=0):
    """pn2_cluster_points -> ids (n,) int32, header (8,) int32, both checked to stay inside their guards, the inputs unchanged"""
    import torch
    lib = pn2._lib
    n = len(pts)
    d_pts = torch.from_numpy(pts).to(dev)
    d_lab = None if labels is None else torch.from_numpy(labels).to(dev)
    raw_ids, ids = _guarded(torch, dev, 4 * n)
    raw_hdr, hdr = _guarded(torch, dev, 32)
    ws, ws_ptr, ws_bytes = _workspace(torch, pn2, dev, n)
    lib.launch("pn2_cluster_points", dev, n, lib.ptr(d_pts), lib.ptr(d_lab), float(eps), min_points, max_points, lib.ptr(ids),
               lib.ptr(hdr), ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes(), "points changed"
    assert labels is None or d_lab.cpu().numpy().tobytes() == labels.tobytes(), "labels changed"
    return _payload(raw_ids, 4 * n, "ids").view(np.int32), _payload(raw_hdr, 32, "header").view(np.int32)


def _stats(pn2, dev, pts, ids, count, labels=None):
    """pn2_cluster_stats -> first, size, label, bbox"""
    import torch
    lib = pn2._lib
    n = len(pts)
    d_pts, d_ids = torch.from_numpy(pts).to(dev), torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    d_lab = None if labels is None else torch.from_numpy(labels).to(dev)
    outs = [_guarded(torch, dev, nb) for nb in (4 * count, 4 * count, 4 * count, 24 * count)]
    lib.launch("pn2_cluster_stats", dev, n, count, lib.ptr(d_pts), lib.ptr(d_lab), lib.ptr(d_ids), *[lib.ptr(v) for _, v in outs])
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes() and d_ids.cpu().numpy().tobytes() == ids.tobytes(), "inputs changed"
    assert labels is None or d_lab.cpu().numpy().tobytes() == labels.tobytes(), "labels changed"
    first, size, label = (_payload(raw, 4 * count, w).view(np.int32) for (raw, _), w in zip(outs, ("first", "size", "label")))
    return first, size, label, _payload(outs[3][0], 24 * count, "bbox").view(np.float32).reshape(count, 6)


def _colors(pn2, dev, ids):
    import torch
    lib = pn2._lib
    d_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    raw, rgb = _guarded(torch, dev, 3 * len(ids))
    lib.launch("pn2_cluster_colors", dev, len(ids), lib.ptr(d_ids), lib.ptr(rgb))
    torch.cuda.synchronize()
    assert d_ids.cpu().numpy().tobytes() == ids.tobytes(), "ids changed"
    return _payload(raw, 3 * len(ids), "rgb").reshape(len(ids), 3)


def _same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes() == np.ascontiguousarray(b, dtype=np.float32).tobytes()


def _check(pn2, dev, pts, eps, labels=None, min_points=1, max_points=0, stats=True):
    """everything against the model; -> ids, header"""
    ids, hdr = _cluster(pn2, dev, pts, eps, labels, min_points, max_points)
    want_ids, want_hdr = C.cluster(pts, eps, labels, min_points, max_points)
    assert hdr.tolist() == want_hdr.tolist(), "header"
    assert np.array_equal(ids, want_ids), "%d ids differ" % (ids != want_ids).sum()
    if stats and hdr[1]:
        got = _stats(pn2, dev, pts, ids, int(hdr[1]), labels)
        want = C.stats(pts, want_ids, labels, int(hdr[1]))
        for g, w, what in zip(got[:3], want[:3], ("first", "size", "label")):
            assert np.array_equal(g, w), what
        assert _same_bits(got[3], want[3]), "bbox"
        assert int(got[1].sum()) == hdr[4]
    return ids, hdr


def _known(groups, valid=None, min_points=1, max_points=0):
    """the answer for a cloud whose components are known by construction: groups (n,) any integers, one per component
    -> ids, header (numpy only, without the model)"""
    n = len(groups)
    valid = np.ones(n, dtype=bool) if valid is None else valid
    _, inv = np.unique(groups, return_inverse=True)
    first = np.full(inv.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, inv[valid], np.nonzero(valid)[0])
    size = np.bincount(inv[valid], minlength=len(first))
    exists = size > 0
    kept = exists & (size >= min_points) & ((size <= max_points) if max_points else True)
    rank = np.full(len(first), -1, dtype=np.int64)
    order = np.argsort(np.where(kept, first, n + 1), kind="stable")[:kept.sum()]
    rank[order] = np.arange(kept.sum())
    ids = np.where(valid, rank[inv], -1).astype(np.int32)
    return ids, np.array([0, kept.sum(), exists.sum(), valid.sum(), size[kept].sum(), 0, 0, 0], dtype=np.int32)


def _cube(seed, n):
    """n points at the density of 4000 in a unit cube: at eps = 0.05 a mix of singletons and small components, at 0.06 one that
    holds most of the cloud"""
    rs = np.random.RandomState(seed)
    return (rs.random_sample((n, 3)) * (n / 4000.0) ** (1.0 / 3.0)).astype(np.float32)


# ---- sizes around wave, workgroup and scan-block edges -----------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.05, 0.06])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4000])
def test_sizes_against_the_model(pn2, cuda, n, eps):
    ids, hdr = _check(pn2, cuda, _cube(n, n), eps)
    if n == 4000:  # the mix the shapes were chosen for
        sizes = np.bincount(ids)
        assert (hdr[1] > 1000 and sizes.max() > 50 and (sizes == 1).sum() > 300) if eps == 0.05 else sizes.max() > 2000


def test_more_blocks_than_one_pass_of_the_block_scan(pn2, cuda):
    """BLOCK * BLOCK + 1 points: the block counts no longer fit one pass of the one-workgroup scan.  Coincident pairs 2.0 apart
    (index 2k and 2k + 1 before the shuffle) and one point left over, min_points = 2: known without the model"""
    n = BLOCK * BLOCK + 1
    rs = np.random.RandomState(11)
    group = np.arange(n) // 2
    pts = np.stack([(group % 256) * 2.0 - 100.5, (group // 256) * 2.0 + 0.25, np.full(n, -3.0)], 1).astype(np.float32)
    order = rs.permutation(n)
    pts, group = np.ascontiguousarray(pts[order]), group[order]
    for min_points in (1, 2):
        ids, hdr = _cluster(pn2, cuda, pts, 0.5, None, min_points)
        want_ids, want_hdr = _known(group, None, min_points)
        assert hdr.tolist() == want_hdr.tolist() and np.array_equal(ids, want_ids)
    assert want_hdr[1] == n // 2 and want_hdr[2] == n // 2 + 1 and want_hdr[4] == n - 1


# ---- the threshold -----------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive_and_exact(pn2, cuda):
    pair = np.zeros((2, 3), dtype=np.float32)
    pair[1, 0] = 0.5
    assert _check(pn2, cuda, pair, 0.5)[0].tolist() == [0, 0]
    pair[1, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    assert _check(pn2, cuda, pair, 0.5)[0].tolist() == [0, 1]
    # 3-4-5 scaled by 0.1: 0.3, 0.4 and 0.5 are not exact and neither are their squares: whatever the fixed formula gives
    for scale in (0.1, 0.7, 1.0, 1e-3, 123.456):
        tri = np.array([[0, 0, 0], [3 * scale, 4 * scale, 0], [0, -4 * scale, 3 * scale]], dtype=np.float32)
        _check(pn2, cuda, tri, np.float32(5 * scale))
    # a contracted multiply-add would decide these differently from the model now and then
    rs = np.random.RandomState(3)
    a = rs.random_sample((600, 3)).astype(np.float32)
    d = rs.standard_normal((600, 3))
    b = (a + 0.125 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)  # partners 0.125 away, to rounding
    pts = np.ascontiguousarray(np.concatenate([a + np.arange(600)[:, None] * np.float32(2.0), b + np.arange(600)[:, None] * np.float32(2.0)])
                               .astype(np.float32))
    ids, hdr = _check(pn2, cuda, pts, 0.125, stats=False)
    assert 600 < hdr[1] < 1200  # some pairs inside, some outside


# ---- a long chain ------------------------------------------------------------------------------------------------------------
def test_long_chain_in_shuffled_order(pn2, cuda):
    n = 4097
    rs = np.random.RandomState(5)
    order = rs.permutation(n)
    pts = np.zeros((n, 3), dtype=np.float32)
    pts[order, 0] = np.arange(n) * 0.5 - 1000.25  # multiples of 0.5, offset: exact, spaced exactly eps
    ids, hdr = _check(pn2, cuda, pts, 0.5)
    assert (ids == 0).all() and hdr.tolist() == [0, 1, 1, n, n, 0, 0, 0]
    first, size, _, bbox = _stats(pn2, cuda, pts, ids, 1)
    assert first.tolist() == [0] and size.tolist() == [n] and bbox.tolist() == [[-1000.25, 0, 0, 1047.75, 0, 0]]
    # one point taken out of the chain: two components
    gone = order[1500]
    cut = np.ascontiguousarray(np.delete(pts, gone, axis=0))
    ids, hdr = _check(pn2, cuda, cut, 0.5)
    assert hdr.tolist() == [0, 2, 2, n - 1, n - 1, 0, 0, 0] and sorted(np.bincount(ids).tolist()) == [1500, n - 1501]


# ---- cell edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.5, 0.3, 0.013])
def test_pairs_across_cell_edges(pn2, cuda, eps):
    """pairs that straddle k * eps and the grid's own cell edges (origin + m * h, h = eps * (1 + 2^-20), the origin no multiple of
    eps and negative) from either side, the nearer point on the edge or one ulp off it, the two eps apart or one ulp less or more:
    every pair within eps must be found, whatever cells the two fall into (the model knows no cells)"""
    e = np.float32(eps)
    origin = np.array([-7.3, -8.9, -9.77], dtype=np.float32) * e  # the minimum of the cloud on every axis
    h = np.float64(e) * (1.0 + 2.0 ** -20)
    step = np.float32(40.0) * e  # a pair meets no other pair
    pts = [origin]
    for axis in range(3):
        edges = [np.float32(k) * e for k in (-3, -1, 0, 1, 2, 5, 17)]
        edges += [np.float32(np.float64(origin[axis]) + m * h) for m in (1, 2, 5, 17, 300)]
        for edge in edges:
            for shift in (-1, 0, 1):
                at = edge if shift == 0 else np.nextafter(edge, np.float32(shift * np.inf))
                for reach in (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1)), -e):
                    near = np.zeros(3, dtype=np.float32)
                    near[(axis + 1) % 3] = step * np.float32(len(pts))
                    near[axis] = at
                    far = near.copy()
                    far[axis] = at + reach  # rounded to float32: the model decides what that makes of the pair
                    pts += [near, far]
    pts = np.ascontiguousarray(np.array(pts, dtype=np.float32))
    assert (pts >= origin).all()
    ids, hdr = _check(pn2, cuda, pts, e)
    assert len(pts) // 2 < hdr[1] < len(pts)  # some pairs linked, some not


# ---- crowded cells -------------------------------------------------------------------------------------------------------------
def test_crowded_cells(pn2, cuda):
    same = np.tile(np.array([[1.5, -2.25, 0.125]], dtype=np.float32), (300, 1))  # more than a workgroup in one cell
    ids, hdr = _check(pn2, cuda, same, 0.01)
    assert (ids == 0).all() and hdr.tolist() == [0, 1, 1, 300, 300, 0, 0, 0]
    rs = np.random.RandomState(8)
    cloud = (rs.random_sample((2000, 3)) - 0.5).astype(np.float32)
    ids, hdr = _check(pn2, cuda, cloud, 4.0)  # eps larger than the cloud: one cell
    assert (ids == 0).all() and hdr[1] == 1


# ---- labels and validity -------------------------------------------------------------------------------------------------------
def test_labels_keep_classes_apart(pn2, cuda):
    rs = np.random.RandomState(9)
    half = _cube(9, 700)
    pts = np.ascontiguousarray(np.repeat(half, 2, axis=0))  # two classes interleaved at the same positions
    labels = np.tile(np.array([3, 5], dtype=np.int32), 700)
    ids, hdr = _check(pn2, cuda, pts, 0.06, labels)
    assert set(ids[0::2]).isdisjoint(ids[1::2])
    one, hdr_one = _check(pn2, cuda, half, 0.06)
    assert hdr[1] == 2 * hdr_one[1]
    labels = rs.randint(-1, 3, 1400).astype(np.int32)  # -1 excludes
    ids, hdr = _check(pn2, cuda, pts, 0.06, labels)
    assert (ids[labels < 0] == -1).all() and (ids[labels >= 0] >= 0).all() and hdr[3] == (labels >= 0).sum()


def test_non_finite_points_are_left_out(pn2, cuda):
    pts = _cube(10, 500) + np.float32(3.0)
    clean_ids, _ = _check(pn2, cuda, pts, 0.06)
    bad = pts.copy()
    bad[100, 0], bad[200, 1], bad[300, 2] = np.nan, np.inf, -np.inf  # -inf would drag the grid's origin if it were read
    ids, hdr = _check(pn2, cuda, bad, 0.06)
    assert ids[[100, 200, 300]].tolist() == [-1, -1, -1] and hdr[0] == 0 and hdr[3] == 497
    keep = np.ones(500, dtype=bool)
    keep[[100, 200, 300]] = False
    again, _ = _check(pn2, cuda, np.ascontiguousarray(pts[keep]), 0.06)
    assert np.array_equal(ids[keep], again)
    everything = np.full((70, 3), np.nan, dtype=np.float32)  # no valid point at all
    ids, hdr = _check(pn2, cuda, everything, 0.06)
    assert (ids == -1).all() and hdr.tolist() == [0] * 8


# ---- the size filter -----------------------------------------------------------------------------------------------------------
def test_size_filter_and_numbering(pn2, cuda):
    rs = np.random.RandomState(12)
    sizes = [1, 2, 3, 4, 5, 6, 7, 3, 4, 6, 7, 1, 5]
    group = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    pts = np.zeros((len(group), 3), dtype=np.float32)
    pts[:, 1] = group * 3.0 - 7.0  # coincident members, components 3.0 apart
    for min_points, max_points in ((4, 6), (4, 0), (1, 3), (7, 7), (8, 0), (1, 0)):  # sizes min - 1, min, max, max + 1 all occur
        ids, hdr = _check(pn2, cuda, pts, 1.0, None, min_points, max_points)
        want_ids, want_hdr = _known(group, None, min_points, max_points)
        assert np.array_equal(ids, want_ids) and hdr.tolist() == want_hdr.tolist()
        firsts = [np.nonzero(ids == c)[0][0] for c in range(hdr[1])]
        assert firsts == sorted(firsts)
        if min_points == 8:
            assert hdr[1] == 0 and (ids == -1).all() and hdr[2] == len(sizes)


# ---- status and errors ---------------------------------------------------------------------------------------------------------
def test_status_too_many_cells(pn2, cuda):
    import torch
    pts = np.array([[0, 0, 0], [1e6, 0, 0]], dtype=np.float32)
    ids, hdr = _cluster(pn2, cuda, pts, 0.1)
    assert ids.tolist() == [-1, -1] and hdr.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="2\\^21 cells"):
        pn2.euclidean_clusters(torch.from_numpy(pts).to(cuda), 0.1)
    pts[1, 0] = 2.0e5  # 2 * 10^6 cells: just inside
    assert _check(pn2, cuda, pts, 0.1)[1].tolist() == [0, 2, 2, 2, 2, 0, 0, 0]


def test_linked_pair_in_the_last_two_cells_of_every_axis(pn2, cuda):
    """the top edge of the grid: with eps = 1 and the minimum pinned at the origin, cell c of an axis is [c * h, (c + 1) * h),
    h = 1 + 2^-20, so 2097152.75 lies in cell 2^21 - 2 and 2097153.25 in cell 2^21 - 1, the last one (float32 resolves 0.25
    there); the diagonal pair is 0.5 * sqrt(3) apart: linked, and the walk of the later point clamps x at the grid's edge"""
    a, b = 2097152.75, 2097153.25
    pts = np.array([[0, 0, 0], [a, a, a], [b, b, b]], dtype=np.float32)
    cells = np.floor(pts.astype(np.float64) / (1.0 + 2.0 ** -20))
    assert (cells[1] == 2 ** 21 - 2).all() and (cells[2] == 2 ** 21 - 1).all()
    ids, hdr = _check(pn2, cuda, pts, 1.0)
    assert ids.tolist() == [0, 1, 1] and hdr.tolist() == [0, 2, 2, 3, 3, 0, 0, 0]


def test_refusals_leave_the_outputs_untouched(pn2, cuda):
    import torch
    lib, K = pn2._lib, pn2._lib.ABI.constants
    n = 100
    d_pts = torch.zeros((n, 3), dtype=torch.float32, device=cuda)
    d_lab = torch.zeros((n,), dtype=torch.int32, device=cuda)
    raw_ids, ids = _guarded(torch, cuda, 4 * n)
    raw_hdr, hdr = _guarded(torch, cuda, 32)
    ws, ws_ptr, ws_bytes = _workspace(torch, pn2, cuda, n)
    good = dict(n=n, points=lib.ptr(d_pts), labels=lib.ptr(d_lab), eps=0.5, min_points=1, max_points=0, ids=lib.ptr(ids),
                header=lib.ptr(hdr), workspace=ws_ptr, workspace_bytes=ws_bytes, stream=lib.stream_ptr())
    names = lib.ABI.functions["pn2_cluster_points"].argnames
    cases = [(dict(n=0), "EINVAL"), (dict(n=-1), "EINVAL"), (dict(eps=0.0), "EINVAL"), (dict(eps=-0.5), "EINVAL"),
             (dict(eps=float("nan")), "EINVAL"), (dict(eps=float("inf")), "EINVAL"), (dict(min_points=0), "EINVAL"),
             (dict(max_points=-1), "EINVAL"), (dict(points=None), "ENULL"), (dict(ids=None), "ENULL"), (dict(header=None), "ENULL"),
             (dict(workspace=None), "ENULL"), (dict(workspace_bytes=ws_bytes - 512), "EINVAL"), (dict(workspace_bytes=0), "EINVAL"),
             (dict(workspace=ws_ptr + 4), "EINVAL")]
    with torch.cuda.device(cuda):
        for change, code in cases:
            a = dict(good, **change)
            assert lib.lib.pn2_cluster_points(*[a[k] for k in names]) == K["PN2_" + code], change
    torch.cuda.synchronize()
    assert (_payload(raw_ids, 4 * n, "ids") == POISON).all() and (_payload(raw_hdr, 32, "header") == POISON).all()
    assert (ws.cpu().numpy() == POISON).all(), "the workspace was written"


# ---- large, known by construction ----------------------------------------------------------------------------------------------
def test_lattice_of_blobs(pn2, cuda):
    """about 70 000 points: blobs of 1 to 600 points inside cubes of side 0.1 (eps = 0.2 joins every two points of one) on a lattice
    of spacing 1, shuffled: ids, sizes and boxes are known without the model"""
    rs = np.random.RandomState(13)
    sizes = 1 + (np.arange(233) * 37) % 600
    sizes[7], sizes[100] = 1, 600
    group = np.repeat(np.arange(len(sizes)), sizes)
    n = len(group)
    assert 60000 < n < 80000
    site = np.stack([group % 8, (group // 8) % 8, group // 64], 1) - 3.5
    pts = (site + rs.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)
    labels = (group % 4).astype(np.int32)
    order = rs.permutation(n)
    pts, group, labels = np.ascontiguousarray(pts[order]), group[order], np.ascontiguousarray(labels[order])
    for lab in (None, labels):
        ids, hdr = _cluster(pn2, cuda, pts, 0.2, lab, 1, 0)
        want_ids, want_hdr = _known(group)
        assert hdr.tolist() == want_hdr.tolist() and np.array_equal(ids, want_ids)
    ids, hdr = _cluster(pn2, cuda, pts, 0.2, labels, 20, 500)
    want_ids, want_hdr = _known(group, None, 20, 500)
    assert hdr.tolist() == want_hdr.tolist() and np.array_equal(ids, want_ids)
    count = int(hdr[1])
    first, size, label, bbox = _stats(pn2, cuda, pts, ids, count, labels)
    assert int(size.sum()) == hdr[4]
    for c in range(0, count, 7):
        at = np.nonzero(want_ids == c)[0]
        assert first[c] == at[0] and size[c] == len(at) and label[c] == labels[at[0]]
        assert _same_bits(bbox[c], np.concatenate([pts[at].min(axis=0), pts[at].max(axis=0)]))  # numpy's own min and max
    assert np.array_equal(size, np.bincount(want_ids[want_ids >= 0])) and (np.diff(first) > 0).all()


# ---- stats and colours ---------------------------------------------------------------------------------------------------------
def test_stats_and_colors_against_the_model(pn2, cuda):
    rs = np.random.RandomState(14)
    n = 3000
    pts = (rs.standard_normal((n, 3)) * 50).astype(np.float32)
    pts[::17] = 0.0
    pts[5::17, 1] = -0.0  # signed zeros: -0.0 is the smaller
    labels = rs.randint(0, 9, n).astype(np.int32)
    count = 41
    ids = rs.randint(-1, count, n).astype(np.int32)
    ids[:count] = np.arange(count)[::-1]  # every cluster has a point
    got = _stats(pn2, cuda, pts, ids, count, labels)
    want = C.stats(pts, ids, labels, count)
    for g, w, what in zip(got[:3], want[:3], ("first", "size", "label")):
        assert np.array_equal(g, w), what
    assert _same_bits(got[3], want[3])
    assert got[2].tolist() == labels[got[0]].tolist() and _stats(pn2, cuda, pts, ids, count)[2].tolist() == [0] * count
    # an id beyond the tables is ignored, never written
    wild = ids.copy()
    wild[count:count + 5] = [count, count + 1, 10 ** 6, 2 ** 31 - 1, -7]
    inside = wild.copy()
    inside[count:count + 5] = -1
    for g, w in zip(_stats(pn2, cuda, pts, wild, count, labels), C.stats(pts, inside, labels, count)):
        assert g.tobytes() == w.tobytes()
    for some in (np.arange(-1, 300, dtype=np.int32), ids, np.array([2 ** 31 - 1, -2 ** 31, -1, 0], dtype=np.int32),
                 np.arange(BLOCK + 1, dtype=np.int32) * 7919):
        assert np.array_equal(_colors(pn2, cuda, some), C.colors(some))


# ---- the wrapper, the KITTI method, the example ----------------------------------------------------------------------------------
def test_wrapper_and_kitti_method(pn2, cuda):
    import torch
    rs = np.random.RandomState(15)
    n = 2500
    pts64 = np.concatenate([rs.random_sample((n - 500, 3)) * [12.0, 12.0, 0.5], rs.random_sample((500, 3)) * 0.3 + [20, 20, 0]])
    labels64 = rs.randint(0, 9, n).astype(np.int64)
    pts32 = pts64.astype(np.float32)
    want_lab = np.where(np.isin(labels64, [8, 2]), labels64, -1).astype(np.int32)
    want_ids, want_hdr = C.cluster(pts32, 0.5, want_lab, 3, 200)
    want = C.stats(pts32, want_ids, want_lab, int(want_hdr[1]))
    assert want_hdr[1] > 3

    def same(c):
        assert isinstance(c, pn2.Clusters) and c.count == want_hdr[1] and c.ids.dtype == torch.int32 and c.ids.device == cuda
        assert np.array_equal(c.ids.cpu().numpy(), want_ids)
        for g, w in zip((c.first, c.size, c.label), want[:3]):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
        assert c.bbox.dtype == torch.float32 and _same_bits(c.bbox.cpu().numpy(), want[3])

    same(pn2.euclidean_clusters(pts64, 0.5, labels=labels64, classes=(8, 2), min_points=3, max_points=200))  # numpy, float64
    d_pts, d_lab = torch.from_numpy(pts64).to(cuda), torch.from_numpy(labels64).to(cuda)
    same(pn2.euclidean_clusters(d_pts, 0.5, labels=d_lab, classes=iter([2, 8, 8]), min_points=3, max_points=200))  # tensors
    frame = types.SimpleNamespace(points=d_pts.float())
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)  # the method uses none of the network's state
    same(predictor.objects_for_frame(frame, d_lab.to(torch.int32), 0.5, [8, 2], min_points=3, max_points=200))
    # nothing kept, nothing there, and no labels
    none = pn2.euclidean_clusters(d_pts, 0.5, labels=d_lab, classes=[8], min_points=10 ** 6)
    assert none.count == 0 and (none.ids == -1).all() and none.first.shape == (0,) and none.bbox.shape == (0, 6)
    empty = pn2.euclidean_clusters(d_pts[:0], 0.5)
    assert empty.count == 0 and empty.ids.shape == (0,) and empty.bbox.shape == (0, 6)
    plain = pn2.euclidean_clusters(d_pts, 0.5, max_points=None)
    ids, hdr = C.cluster(pts32, 0.5)
    assert plain.count == hdr[1] and np.array_equal(plain.ids.cpu().numpy(), ids) and (plain.label == 0).all()
    rgb = pn2.cluster_colors(plain.ids)
    assert rgb.dtype == torch.uint8 and np.array_equal(rgb.cpu().numpy(), C.colors(ids))
    assert np.array_equal(pn2.cluster_colors(plain.ids.long()).cpu().numpy(), C.colors(ids))
    image = pn2.render.render_colors(d_pts.float(), rgb, "top", 160, 120)
    assert tuple(image.shape) == (120, 160, 3)


def test_example_on_a_synthetic_scene(pn2, cuda, tmp_path):
    n = 3000
    out = str(tmp_path / "objects")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_objects.py"), "--synthetic", str(n), "--out", out,
                          "--min_points", "5", "--width", "320", "--height", "200"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    spec = importlib.util.spec_from_file_location("cluster_objects_example", os.path.join(ROOT, "examples", "cluster_objects.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    pts, labels = example.synthetic(n)
    ids, hdr = C.cluster(pts, example.SYNTHETIC_EPS, labels, 5, 0)
    first, size, label, bbox = C.stats(pts, ids, labels, int(hdr[1]))
    want = ["%d %d %d %s" % (c, label[c], size[c], " ".join(repr(float(v)) for v in bbox[c])) for c in range(hdr[1])]
    with open(os.path.join(out, "objects.txt")) as f:
        assert f.read().splitlines() == want
    # the blobs themselves: 1 + 37 k mod 60 points each, those of 5 and more are kept
    blob_sizes = []
    while sum(blob_sizes) < n:
        blob_sizes.append(min(1 + (37 * len(blob_sizes)) % 60, n - sum(blob_sizes)))
    assert sorted(size.tolist()) == sorted(s for s in blob_sizes if s >= 5)
    for c in (1, 2, 3):
        assert "class %d: %d objects" % (c, (label == c).sum()) in run.stdout
    with open(os.path.join(out, "objects.png"), "rb") as f:
        png = f.read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (320, 200)
