"""GPU tests of object description: pn2_cluster_describe / pn2_box_wireframe (csrc/pn2_describe.hip) against the numpy model of the
rules (tests/describe_ref.py); every output between poisoned guards, every input compared unchanged, the workspace poisoned;
pn2.cluster's wrapper, the KITTI method and examples/cluster_objects.py --boxes.

There is no tolerance anywhere: the moments are integer sums, the extents integer minima / maxima of ordered keys, and everything
between them is float64 in a fixed association without contraction, with correctly rounded sqrt and division.  moments and desc
are compared with the model bit for bit, for both values of upright.  Nothing here captures a graph.

The kernels handle one point (or one cluster) per thread and loop over nothing, so there is no chunk count to walk: the sizes
below are chosen around the wave (64), the workgroup (BLOCK) and the peel threshold (MIN_LANES) instead."""
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
import describe_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64       # guard bytes in front of and behind every output
WAVE = 64
BLOCK = 256  # kT of csrc/pn2_describe.hip: threads per workgroup = points per workgroup
MIN_LANES = 2  # kPeelMinLanes of csrc/pn2_describe.hip: an id held by at least this many lanes of a wave is reduced inside the
               # wave, the lanes of an id held by fewer issue their own atomics (kPeelRounds = 64: every id of a wave is looked at)


def _guarded(torch, dev, nbytes):
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _describe(pn2, dev, pts, ids, count, upright):
    """pn2_cluster_describe -> moments (count,12) int64, desc (count,24) float64: inside their guards, the inputs unchanged"""
    import torch
    lib = pn2._lib
    n = len(pts)
    d_pts, d_ids = torch.from_numpy(pts).to(dev), torch.from_numpy(ids).to(dev)
    raw_m, mom = _guarded(torch, dev, 96 * count)
    raw_d, desc = _guarded(torch, dev, 192 * count)
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_cluster_describe_workspace_size", dev, count, ctypes.byref(nbytes), stream=False)
    ws = torch.full((int(nbytes.value) + 255 + G,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    lib.launch("pn2_cluster_describe", dev, n, count, lib.ptr(d_pts), lib.ptr(d_ids), upright, lib.ptr(mom), lib.ptr(desc),
               ws.data_ptr() + off, int(nbytes.value))
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes() and d_ids.cpu().numpy().tobytes() == ids.tobytes(), "inputs changed"
    assert (ws[off + int(nbytes.value):] == POISON).all(), "written behind the workspace"
    return (_payload(raw_m, 96 * count, "moments").view(np.int64).reshape(count, 12),
            _payload(raw_d, 192 * count, "desc").view(np.float64).reshape(count, 24))


def _check(pn2, dev, pts, ids, count):
    """both values of upright against the model, bit for bit -> the model's (moments, desc) for upright = 0"""
    pts, ids = np.ascontiguousarray(pts, dtype=np.float32), np.ascontiguousarray(ids, dtype=np.int32)
    out = None
    for upright in (0, 1):
        mom, desc = _describe(pn2, dev, pts, ids, count, upright)
        want_mom, want_desc = D.describe(pts, ids, count, upright)
        assert np.array_equal(mom, want_mom), "moments, upright=%d: rows %s" % (upright, np.nonzero((mom != want_mom).any(1))[0][:8])
        same = desc.view(np.uint64) == want_desc.view(np.uint64)
        assert same.all(), "desc, upright=%d: rows %s columns %s\n%r\n%r" % (
            upright, np.nonzero(~same.all(1))[0][:8], np.nonzero(~same.all(0))[0], desc[~same.all(1)][:2], want_desc[~same.all(1)][:2])
        out = out or (want_mom, want_desc)
    return out


def _blob(rs, m, centre=(0.0, 0.0, 0.0), spread=(2.0, 0.7, 0.3)):
    yaw = rs.uniform(0, np.pi)
    turn = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    return ((rs.standard_normal((m, 3)) * spread) @ turn.T + centre).astype(np.float32)


# ---- cluster sizes around the wave and the workgroup ---------------------------------------------------------------------------
def test_cluster_sizes_in_a_shuffled_cloud(pn2, cuda):
    """clusters of 1, 2, 63, 64, 65 and 257 members and one without any, ids of -1 and >= nclusters, member ids on non-finite
    points; n is no multiple of 64 or 256"""
    rs = np.random.RandomState(0)
    sizes = [1, 2, 63, 64, 65, 257, 0, 5]
    count = len(sizes)
    ids = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(140, -1), [count, count + 1, 10 ** 6, 2 ** 31 - 1, -7]])
    pts = np.concatenate([_blob(rs, s, rs.uniform(-30, 30, 3)) for s in sizes] + [_blob(rs, 145, (1.0, 2.0, 3.0), (50, 50, 50))])
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], dtype=np.float32)
    pts, ids = np.concatenate([pts, bad]), np.concatenate([ids, [5, 5, 3, 0]])  # member ids on non-finite points
    order = rs.permutation(len(ids))
    pts, ids = pts[order], ids[order]
    assert len(ids) % WAVE and len(ids) % BLOCK and len(ids) > 2 * BLOCK
    mom, desc = _check(pn2, cuda, pts, ids, count)
    assert mom[:, 0].tolist() == sizes and np.isnan(desc[6]).all() and not np.isnan(desc[[0, 1, 2, 3, 4, 5, 7]]).any()


# ---- the three paths of a wave: one id, a few ids peeled, one atomic per lane --------------------------------------------------
@pytest.mark.parametrize("layout", ["one id per wave", "64 ids in a wave", "peel threshold", "run across wave and workgroup edges",
                                    "sorted by id", "non-members between"])
def test_wave_layouts(pn2, cuda, layout):
    rs = np.random.RandomState(len(layout))
    if layout == "one id per wave":  # every lane of a wave holds the same id; the last wave is partial
        ids = np.repeat(np.arange(6), WAVE)[:5 * WAVE + 37]
    elif layout == "64 ids in a wave":  # all distinct, then the same 64 again in another order in the next wave
        ids = np.concatenate([np.arange(WAVE), rs.permutation(WAVE), np.arange(WAVE)[:29]])
    elif layout == "peel threshold":
        # per wave, ids held by MIN_LANES - 1, MIN_LANES and MIN_LANES + 1 lanes next to singletons and one large group: reduced
        # and per-lane ids side by side in one wave; the lanes of an id interleaved, in runs, and with the id of the wave before
        def wave(first, shuffle):
            groups = [MIN_LANES - 1, MIN_LANES, MIN_LANES + 1, 1, 1, 1]
            lanes = np.repeat(np.arange(len(groups) + 1), groups + [WAVE - sum(groups)]) + first
            return rs.permutation(lanes) if shuffle else lanes
        ids = np.concatenate([wave(0, False), wave(0, True), wave(3, True), wave(5, False)[::-1],
                              np.arange(WAVE) % (WAVE // MIN_LANES), np.arange(WAVE) % (WAVE // MIN_LANES + 1)])[:-11]
    elif layout == "run across wave and workgroup edges":  # id 1 runs from lane 40 of wave 2 through the workgroup edge at 256
        ids = np.concatenate([np.zeros(2 * WAVE + 40), np.ones(BLOCK), np.full(3 * WAVE + 5, 2)])
    elif layout == "sorted by id":  # what a sorted grid leaves: runs of every length
        ids = np.sort(rs.randint(0, 9, 3 * BLOCK + 77))
    else:  # a wave whose members are few: ids of -1 between them, and a wave without any member
        ids = np.where(rs.random_sample(4 * BLOCK + 3) < 0.2, rs.randint(0, 3, 4 * BLOCK + 3), -1)
        ids[BLOCK:BLOCK + WAVE] = -1
    ids = ids.astype(np.int32)
    count = int(ids.max()) + 1
    centres = rs.uniform(-20, 20, (count, 3))
    pts = (rs.standard_normal((len(ids), 3)) * [1.5, 0.5, 0.2] + centres[np.maximum(ids, 0)]).astype(np.float32)
    mom, _ = _check(pn2, cuda, pts, ids, count)
    assert mom[:, 0].tolist() == np.bincount(ids[ids >= 0], minlength=count).tolist()


# ---- degenerate shapes ---------------------------------------------------------------------------------------------------------
def test_degenerate_clusters(pn2, cuda):
    rs = np.random.RandomState(2)
    line = np.outer(np.arange(20) - 7.0, [0.5, 0.25, -1.0])                                        # collinear
    plane = np.concatenate([rs.randint(-50, 50, (60, 2)) / 8.0, np.full((60, 1), 2.5)], 1)          # planar, z constant
    tilted = np.stack([plane[:, 0], plane[:, 1], plane[:, 0] * 0.5 + plane[:, 1] * 0.25], 1)        # planar, tilted
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)  # equal eigenvalues
    same = np.full((9, 3), [3.5, -2.25, 1e-3])                                                      # E == 0
    one = np.array([[-7.0, 1e10, 3e-20]])                                                           # a single member
    far = rs.random_sample((100, 3)) + [1e6, -1e6, 1e6]                                             # 1 m at 10^6: float32 steps of 1/16
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, -0.0], [-0.0, 0.0, 0.0]])    # E == 0 with signed zeros
    mixed = np.concatenate([zeros, [[-0.0, 1.0, 0.0], [2.0, -0.0, -0.0], [-1.0, 0.0, -0.0]]])       # -0.0 as a minimum and inside
    square = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float64) + [5, 5, 5]  # equal in-plane eigenvalues
    huge = rs.uniform(-1, 1, (30, 3)) * [3e38, 1e-38, 1.0]                                            # the widest E, the narrowest axis
    tiny = rs.randint(0, 4, (30, 3)) * 2.0 ** -149                                                  # subnormal float32 spacing
    parts = [line, plane, tilted, cube, same, one, far, zeros, mixed, square, huge, tiny, cube * 1e-3 + 100.0]
    pts = np.concatenate(parts).astype(np.float32)
    ids = np.repeat(np.arange(len(parts)), [len(p) for p in parts]).astype(np.int32)
    mom, desc = _check(pn2, cuda, pts, ids, len(parts) + 1)  # + one cluster without members
    assert mom[-1].tolist() == [0] * 12 and np.isnan(desc[-1]).all()
    assert mom[4].tolist() == [9] + [0] * 9 + [20, 20] and desc[4, 3:6].tolist() == [0.0] * 3 and desc[4, 15:21].tolist() == [0.0] * 6
    assert desc[0, 3] > 0 and abs(desc[0, 4]) < 1e-9 * desc[0, 3] and abs(desc[0, 5]) < 1e-9 * desc[0, 3]  # a line: one variance
    assert desc[1, 5] == 0.0 and desc[1, 4] > 0                        # a plane: two
    assert desc[3, 3] == desc[3, 4] == desc[3, 5] and desc[3, 6:15].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]  # a cube: no rotation
    # the same again, shuffled, with ids beyond the table in between
    order = rs.permutation(len(ids))
    _check(pn2, cuda, pts[order], ids[order], len(parts) + 1)


def test_two_permutations_give_equal_bits(pn2, cuda):
    """the same cloud in two orders: per cluster every bit of moments and desc is the same (device against device, and both
    against the model inside _check)"""
    rs = np.random.RandomState(3)
    count = 7
    n = 3 * BLOCK + 19
    ids = np.sort(rs.choice(count + 1, n, p=[0.5, 0.2, 0.1, 0.05, 0.05, 0.04, 0.03, 0.03]) - 1).astype(np.int32)
    centres = rs.uniform(-40, 40, (count, 3))
    pts = np.concatenate([_blob(rs, 1, centres[max(c, 0)]) for c in ids])
    pts, ids = np.ascontiguousarray(pts), np.ascontiguousarray(ids)
    order = rs.permutation(n)
    for upright in (0, 1):
        a = _describe(pn2, cuda, pts, ids, count, upright)          # sorted by id: long runs, the wave-reduced path
        b = _describe(pn2, cuda, pts[order].copy(), ids[order].copy(), count, upright)  # shuffled: the peeled and per-lane paths
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _check(pn2, cuda, pts[order], ids[order], count)


def test_many_clusters_more_than_one_workgroup_of_them(pn2, cuda):
    """BLOCK + 3 clusters: the per-cluster kernels run two workgroups; every cluster has a few members, scattered"""
    rs = np.random.RandomState(4)
    count = BLOCK + 3
    ids = np.concatenate([np.arange(count), rs.randint(0, count, 900)]).astype(np.int32)
    pts = (rs.standard_normal((len(ids), 3)) * 0.4 + rs.uniform(-100, 100, (count, 3))[ids]).astype(np.float32)
    order = rs.permutation(len(ids))
    _check(pn2, cuda, pts[order], ids[order], count)


# ---- refusals that need a device -------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(pn2, cuda):
    import torch
    lib = pn2._lib
    pts = torch.zeros((10, 3), dtype=torch.float32, device=cuda)
    ids = torch.zeros((10,), dtype=torch.int32, device=cuda)
    raw_m, mom = _guarded(torch, cuda, 96)
    raw_d, desc = _guarded(torch, cuda, 192)
    ws = torch.full((4096,), POISON, dtype=torch.uint8, device=cuda)
    off = (-ws.data_ptr()) % 256
    call = lib.lib.pn2_cluster_describe
    assert call(10, 1, lib.ptr(pts), lib.ptr(ids), 0, lib.ptr(mom), lib.ptr(desc), ws.data_ptr() + off, 16, lib.stream_ptr()) == -1
    assert call(10, 11, lib.ptr(pts), lib.ptr(ids), 0, lib.ptr(mom), lib.ptr(desc), ws.data_ptr() + off, 2048, lib.stream_ptr()) == -3
    assert call(10, 1, lib.ptr(pts), lib.ptr(ids), 3, lib.ptr(mom), lib.ptr(desc), ws.data_ptr() + off, 2048, lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (raw_m == POISON).all() and (raw_d == POISON).all() and (ws == POISON).all()


# ---- the wireframe -------------------------------------------------------------------------------------------------------------
def _wireframe(pn2, dev, desc, per_edge):
    import torch
    lib = pn2._lib
    count = len(desc)
    d_desc = torch.from_numpy(desc).to(dev)
    total = count * 12 * per_edge
    raw_p, pts = _guarded(torch, dev, 12 * total)
    raw_o, own = _guarded(torch, dev, 4 * total)
    lib.launch("pn2_box_wireframe", dev, count, lib.ptr(d_desc), per_edge, lib.ptr(pts), lib.ptr(own))
    torch.cuda.synchronize()
    assert d_desc.cpu().numpy().tobytes() == desc.tobytes(), "desc changed"
    return _payload(raw_p, 12 * total, "points").view(np.float32).reshape(total, 3), _payload(raw_o, 4 * total, "owner").view(np.int32)


@pytest.mark.parametrize("per_edge", [2, 3, 64])
def test_wireframe_against_the_model(pn2, cuda, per_edge):
    rs = np.random.RandomState(5)
    count = 23  # 23 * 12 * per_edge is no multiple of BLOCK for per_edge = 2, 3
    ids = rs.randint(0, count, 700).astype(np.int32)
    ids[ids == 4] = 5  # a cluster without members: a row of NaNs
    pts = np.concatenate([_blob(rs, 1, (c * 3.0, -c * 2.0, 1.0)) for c in ids])
    for upright in (0, 1):
        _, desc = D.describe(pts, ids, count, upright)
        got_p, got_o = _wireframe(pn2, cuda, np.ascontiguousarray(desc), per_edge)
        want_p, want_o = D.wireframe(desc, per_edge)
        assert np.array_equal(got_o, want_o)
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
        assert np.isnan(got_p[4 * 12 * per_edge:5 * 12 * per_edge]).all() and not np.isnan(got_p[:4 * 12 * per_edge]).any()
    # the ends of every edge are corners of the box, and every corner is the end of three edges
    ends = got_p.reshape(count, 12, per_edge, 3)[0][:, [0, -1]].reshape(24, 3)
    corners = np.array([D.corner(desc[0], j) for j in range(8)]).astype(np.float32)
    assert sorted(map(tuple, ends.tolist())) == sorted(map(tuple, np.repeat(corners, 3, axis=0).tolist()))


# ---- the wrapper, the KITTI method, the example ----------------------------------------------------------------------------------
def test_wrapper_and_kitti_method(pn2, cuda):
    import torch
    rs = np.random.RandomState(6)
    cars = [(4.5, 2.0, 1.6, 0.3, (10, 5, 0.8)), (4.0, 1.8, 1.5, 1.2, (-8, 12, 0.75)), (0.5, 0.5, 1.8, 0.0, (3, -9, 0.9))]
    parts = []
    for length, width, height, yaw, centre in cars:
        box = rs.uniform(-0.5, 0.5, (400, 3)) * [length, width, height]
        turn = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        parts.append(box @ turn.T + centre)
    pts64 = np.concatenate(parts + [rs.uniform(-20, 20, (300, 3)) * [1, 1, 0.01]])
    order = rs.permutation(len(pts64))
    pts64 = pts64[order]
    pts32 = pts64.astype(np.float32)
    d_pts = torch.from_numpy(pts32).to(cuda)
    clusters = pn2.euclidean_clusters(d_pts, 0.6, min_points=100)
    assert clusters.count == 3
    ids = clusters.ids.cpu().numpy()

    def same(b, upright):
        want_mom, want = D.describe(pts32, ids, 3, upright)
        assert isinstance(b, pn2.Boxes) and all(t.device == cuda for t in b)
        assert b.size.dtype == torch.int64 and b.moments.dtype == torch.int64 and np.array_equal(b.moments.cpu().numpy(), want_mom)
        assert b.size.tolist() == clusters.size.tolist()
        got = torch.cat([b.centroid, b.variance, b.axes.reshape(3, 9), b.lo, b.hi, b.center], 1)
        assert got.dtype == torch.float64 and got.cpu().numpy().tobytes() == want.tobytes()
        assert torch.equal(b.extent, b.hi - b.lo) and tuple(b.corners().shape) == (3, 8, 3) and tuple(b.yaw().shape) == (3,)

    for upright in (False, True):
        same(pn2.describe_clusters(d_pts, clusters, upright=upright), int(upright))
    same(pn2.describe_clusters(pts64, (ids.astype(np.int64), 3)), 0)  # numpy, float64 and int64: cast like the clustering does
    same(pn2.describe_clusters(d_pts, (clusters.ids, np.int64(3)), upright=True), 1)
    frame = types.SimpleNamespace(points=d_pts)
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)  # the method uses none of the network's state
    boxes = predictor.describe_objects(frame, clusters)  # upright by default
    same(boxes, 1)
    # the cars come back: size, heading (modulo a half turn) and place, to the sampling of 400 points
    for k, (length, width, height, yaw, centre) in enumerate(cars):
        c = int(ids[np.nonzero(order == 400 * k)[0][0]])  # the cluster of the car's first point
        assert np.abs(boxes.center[c].cpu().numpy() - centre).max() < 0.15
        if k < 2:  # (the post is square: its heading is anybody's guess)
            assert np.abs(boxes.extent[c].cpu().numpy() - [length, width, height]).max() < 0.25
            assert abs((float(boxes.yaw()[c]) - yaw + np.pi / 2) % np.pi - np.pi / 2) < 0.05
    # nothing to describe
    none = pn2.describe_clusters(d_pts, (clusters.ids, 0))
    assert none.size.shape == (0,) and none.axes.shape == (0, 3, 3) and none.moments.shape == (0, 12) and none.size.device == cuda
    # the wireframe, drawn behind the cloud
    edges, owner = pn2.box_wireframe(boxes, per_edge=16)
    _, want = D.describe(pts32, ids, 3, 1)
    want_p, want_o = D.wireframe(want, 16)
    assert edges.dtype == torch.float32 and owner.dtype == torch.int32
    assert np.array_equal(edges.cpu().numpy().view(np.uint32), want_p.view(np.uint32)) and np.array_equal(owner.cpu().numpy(), want_o)
    assert tuple(pn2.box_wireframe(boxes)[0].shape) == (3 * 12 * 64, 3)
    renderer = pn2.render.Renderer(160, 120, device=cuda)
    view = pn2.render.fit_view(d_pts, "top", 160, 120)
    renderer.splat(d_pts, view)
    renderer.splat(edges, view, index0=len(pts32))
    image = renderer.image(torch.cat([pn2.cluster_colors(clusters.ids), pn2.cluster_colors(owner)]))
    assert tuple(image.shape) == (120, 160, 3) and (renderer.indices() >= len(pts32)).sum() > 50  # the edges are seen from above


def test_example_with_boxes(pn2, cuda, tmp_path):
    n = 3000
    out = str(tmp_path / "objects")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_objects.py"), "--synthetic", str(n), "--out", out,
                          "--min_points", "5", "--width", "320", "--height", "200", "--boxes"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    spec = importlib.util.spec_from_file_location("cluster_objects_example", os.path.join(ROOT, "examples", "cluster_objects.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    pts, labels = example.synthetic(n)
    ids, hdr = C.cluster(pts, example.SYNTHETIC_EPS, labels, 5, 0)
    count = int(hdr[1])
    first, size, label, bbox = C.stats(pts, ids, labels, count)
    _, desc = D.describe(pts, ids, count, 1)
    with open(os.path.join(out, "objects.txt")) as f:
        lines = f.read().splitlines()
    assert len(lines) == count
    for c, line in enumerate(lines):
        cols = line.split()
        assert len(cols) == 18
        # the nine columns from before, unchanged
        assert " ".join(cols[:9]) == "%d %d %d %s" % (c, label[c], size[c], " ".join(repr(float(v)) for v in bbox[c]))
        got = [float(v) for v in cols[9:]]
        assert got[0:3] == desc[c, 21:24].tolist() and got[3:6] == (desc[c, 18:21] - desc[c, 15:18]).tolist()  # exact columns
        assert got[6] == pytest.approx(np.arctan2(desc[c, 7], desc[c, 6]), abs=1e-12) and got[7:9] == desc[c, 0:2].tolist()
    for name in ("objects.png", "boxes.png"):
        with open(os.path.join(out, name), "rb") as f:
            png = f.read()
        assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (320, 200)
