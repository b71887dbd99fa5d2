"""GPU tests of fixed-radius neighbourhoods: pn2_radius_neighborhoods (csrc/pn2_neighbors.hip) against the numpy model of the rules
(tests/neighbors_ref.py); every output between poisoned guards, every input compared unchanged, the workspace poisoned;
pn2.neighbors' wrappers, the KITTI method and examples/estimate_normals.py.

There is no tolerance anywhere: a neighbour is decided by one float64 comparison, the moments are integer sums, and everything
after them is float64 in a fixed association without contraction, with correctly rounded sqrt and division.  Every output is
compared with the model bit for bit.  Nothing here captures a graph.

The model is brute force and a Python loop per point, so a case has a few hundred points; the one large case knows its answer
by construction.  Clouds are laid out by CELL (edge radius * (1 + 2^-20), counted from the cloud's minimum) so that the sorted
order, and with it what each wave of the scan holds, is known: the comments say which path a wave takes."""
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
import neighbors_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64       # guard bytes in front of and behind every output
# the constants of csrc/pn2_neighbors.hip (and pn2_cell_grid.h), mirrored:
WAVE = 64    # lanes of a wave: one sorted point each
BLOCK = 256  # kT: threads per workgroup = sorted points per workgroup
CHUNK = 64   # kChunk: candidates per round of the wave-uniform path
SPAN = 8     # kSpan: the widest cx_max - cx_min of a wave that takes the wave-uniform path


def _guarded(torch, dev, nbytes):
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _view(viewpoint):
    return None if viewpoint is None else (ctypes.c_double * 3)(*viewpoint)


def _run(pn2, dev, pts, labels, radius, min_neighbors, viewpoint=None, moments=True, variance=True):
    """pn2_radius_neighborhoods -> neighbors_ref.Result (moments / variance None when not asked for): every output inside its
    guards, the inputs unchanged, nothing written behind the workspace"""
    import torch
    lib = pn2._lib
    n = len(pts)
    d_pts = torch.from_numpy(pts).to(dev)
    d_lab = None if labels is None else torch.from_numpy(labels).to(dev)
    sizes = dict(count=4 * n, moments=72 * n, normals=12 * n, curvature=4 * n, variance=24 * n, header=32)
    raw, out = {}, {}
    for name, nbytes in sizes.items():
        if (name == "moments" and not moments) or (name == "variance" and not variance):
            raw[name], out[name] = None, None
        else:
            raw[name], out[name] = _guarded(torch, dev, nbytes)
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_radius_workspace_size", dev, n, ctypes.byref(nbytes), stream=False)
    ws = torch.full((int(nbytes.value) + 255 + G,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    lib.launch("pn2_radius_neighborhoods", dev, n, lib.ptr(d_pts), lib.ptr(d_lab), float(np.float32(radius)), min_neighbors,
               _view(viewpoint), lib.ptr(out["count"]), lib.ptr(out["moments"]), lib.ptr(out["normals"]), lib.ptr(out["curvature"]),
               lib.ptr(out["variance"]), lib.ptr(out["header"]), ws.data_ptr() + off, int(nbytes.value))
    torch.cuda.synchronize()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes(), "points changed"
    assert labels is None or d_lab.cpu().numpy().tobytes() == labels.tobytes(), "labels changed"
    assert (ws[off + int(nbytes.value):] == POISON).all(), "written behind the workspace"
    got = {name: None if raw[name] is None else _payload(raw[name], nbytes, name) for name, nbytes in sizes.items()}
    return N.Result(got["count"].view(np.int32), None if got["moments"] is None else got["moments"].view(np.int64).reshape(n, 9),
                    got["normals"].view(np.float32).reshape(n, 3), got["curvature"].view(np.float32),
                    None if got["variance"] is None else got["variance"].view(np.float64).reshape(n, 3), got["header"].view(np.int32))


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    same = got.view(np.uint8).reshape(len(got), -1) == want.view(np.uint8).reshape(len(want), -1) if len(got) else np.ones((0, 1), bool)
    rows = np.nonzero(~same.all(1))[0]
    assert len(rows) == 0, "%s: rows %s\n%r\n%r" % (what, rows[:8], got[rows[:3]], want[rows[:3]])


def _check(pn2, dev, pts, radius, labels=None, min_neighbors=3, viewpoint=None):
    """the library against the model, bit for bit -> the model's Result"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    got = _run(pn2, dev, pts, labels, radius, min_neighbors, viewpoint)
    want = N.neighborhoods(pts, radius, labels, min_neighbors, viewpoint)
    assert got.header.tolist() == want.header.tolist()
    for name in ("count", "moments", "normals", "curvature", "variance"):
        _same_bits(getattr(got, name), getattr(want, name), name)
    return want


def _in_cell(rs, m, cell, radius, fill=0.9):
    """m points inside the cell (cx, cy, cz) of a grid of edge `radius` whose minimum is the origin: each coordinate in
    [c + 0.05, c + 0.05 + fill) * radius, well inside the cell whatever the hair on its edge"""
    return (np.asarray(cell, dtype=np.float64) + 0.05 + rs.uniform(0, fill, (m, 3))) * radius


ORIGIN = np.zeros((1, 3))  # a point at the grid's minimum, so that the cells of _in_cell are what they say


# ---- the wrappers' workspace ---------------------------------------------------------------------------------------------------
def test_lib_workspace_is_aligned_and_large_enough(pn2, cuda):
    """_lib.workspace: the size query asked through launch, a 256-aligned uint8 view of at least that many bytes"""
    import torch
    for n in (1, 1000):
        nbytes = ctypes.c_ulonglong(0)
        pn2._lib.launch("pn2_radius_workspace_size", cuda, n, ctypes.byref(nbytes), stream=False)
        ws = pn2._lib.workspace("pn2_radius_workspace_size", cuda, n)
        assert ws.dtype == torch.uint8 and ws.device == torch.device(cuda) and ws.dim() == 1
        assert ws.data_ptr() % 256 == 0 and ws.numel() >= int(nbytes.value) > 0


# ---- the wave-uniform path: chunk edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges_of_the_uniform_path(pn2, cuda, m):
    """one dense blob inside one cell: every wave lies in one row with span 0, and its own row's range holds m candidates --
    1, 63, 64, 65, 129: no chunk, one short of one, exactly one, one and a candidate, two and a candidate"""
    rs = np.random.RandomState(m)
    want = _check(pn2, cuda, _in_cell(rs, m, (0, 0, 0), 0.5), 0.5)
    assert want.header[1] == m and (m == 1 or want.count.min() < m)  # not everybody is everybody's neighbour: the test decides


# ---- which path a wave takes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["two rows in a wave", "span at the limit", "one point per cell", "invalid lanes are loaders"])
def test_choice_of_path(pn2, cuda, layout):
    rs = np.random.RandomState(len(layout))
    radius, labels = 0.75, None
    if layout == "two rows in a wave":
        # 40 points in cell (0,0,0), 40 in (0,1,0): wave 0 holds 40 + 24 and straddles the rows (lane path), wave 1 the last 16
        # of the second row (uniform path); the two blobs are neighbours across the cell edge
        pts = np.concatenate([_in_cell(rs, 40, (0, 0, 0), radius), _in_cell(rs, 40, (0, 1, 0), radius)])
        pts[0] = 0.05 * radius  # (the grid's minimum: the cells are what _in_cell says)
    elif layout == "span at the limit":
        # wave 0: 64 points of the row (y 0, z 0) over the cells x = 0 .. SPAN (uniform path, its ranges SPAN + 3 cells wide);
        # wave 1: 64 points of the row (y 0, z 4) over x = 0 .. SPAN + 1 (lane path)
        def row(z, cells):
            per = WAVE // cells
            return [_in_cell(rs, per + (WAVE - per * cells if c == 0 else 0), (c, 0, z), radius) for c in range(cells)]
        pts = np.concatenate(row(0, SPAN + 1) + row(4, SPAN + 2))
        pts[0] = 0.05 * radius  # (the grid's minimum: the cells are what _in_cell says)
        assert len(pts) == 2 * WAVE
    elif layout == "one point per cell":
        # a 6 x 6 x 6 lattice of spacing 0.99 radius, half a step inside the grid: cell k holds lattice plane k, every point has
        # its 6 axis partners as neighbours, and a wave's 64 sorted points cover ten rows: every wave takes the lane path
        k = np.arange(6)
        lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
        pts = np.concatenate([ORIGIN, (lattice + 0.5) * (0.99 * radius)])
    else:
        # 70 valid points in one cell, then 10 invalid ones (NaN rows, negative labels) and n = 80: wave 1 holds 6 valid lanes,
        # 10 lanes with the key ~0 and 48 lanes beyond n -- and its candidates are 64 + 6, loaded by all of those lanes alike
        pts = np.concatenate([_in_cell(rs, 70, (0, 0, 0), radius), _in_cell(rs, 10, (0, 0, 0), radius)])
        labels = np.zeros(80, dtype=np.int32)
        labels[70:75] = [-1, -7, -1, -2 ** 31, -1]
        pts[75:] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, 0.1, 0.1]]
        pts[0] = 0.05 * radius  # (the grid's minimum: the cells are what _in_cell says)
        order = rs.permutation(80)  # (invalid rows in between)
        pts, labels = pts[order], labels[order]
        assert len(pts) == 80 and (labels >= 0).sum() == 75
    want = _check(pn2, cuda, pts, radius, labels)
    if layout == "one point per cell":
        assert np.sort(want.count[1:])[-1] == 7 and want.header[3] == 7
    if layout == "invalid lanes are loaders":
        assert want.header[1] == 70 and (want.count == 0).sum() == 10


@pytest.mark.parametrize("n", [1, 2, WAVE - 1, WAVE, WAVE + 1, BLOCK + 1, 2 * BLOCK + 37])
def test_cloud_sizes(pn2, cuda, n):
    """a cloud of a few points per cell, shuffled: waves of both kinds, the last one partial"""
    rs = np.random.RandomState(n)
    side = max(1.0, (n / 6.0) ** (1.0 / 3.0))  # about six points per cell of edge 1
    pts = rs.uniform(0, side, (n, 3)) * [1.0, 1.0, 0.3] + [10.0, -20.0, 5.0]
    want = _check(pn2, cuda, pts, 1.0, min_neighbors=2)
    assert want.header[1] == n


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_the_boundary_is_inclusive(pn2, cuda):
    pts = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 5], [0, -5, 0], [9, 9, 9], [-3, 0, -4]], dtype=np.float32)
    want = _check(pn2, cuda, pts, 5.0, min_neighbors=1)
    assert want.count.tolist() == [5, 2, 2, 2, 1, 2]  # every partner at distance exactly 5 is in
    below = np.nextafter(np.float32(5.0), np.float32(0.0))
    assert _check(pn2, cuda, pts, below, min_neighbors=1).count.tolist() == [1] * 6  # one float32 step less: all out


def test_neighbours_one_cell_away_and_strangers_two_cells_away(pn2, cuda):
    """radius 1: partners in the next cell along every axis and across a corner are found; points two cells apart that miss the
    radius by a hair are not"""
    pts = np.array([[0.0, 0.0, 0.0],
                    [0.95, 0.5, 0.5], [1.9, 0.5, 0.5],        # cells x = 0 and 1, 0.95 apart
                    [0.5, 0.95, 0.5], [0.5, 1.9, 0.5],        # the same along y
                    [0.5, 0.5, 0.95], [0.5, 0.5, 1.9],        # and z
                    [0.9, 0.9, 0.9], [1.4, 1.4, 1.4],         # across a corner: cells (0,0,0) and (1,1,1), 0.866 apart
                    [0.999, 3.5, 3.5], [2.0001, 3.5, 3.5],    # cells x = 0 and 2: 1.0011 apart
                    [3.5, 0.999, 3.5], [3.5, 2.0001, 3.5], [3.5, 3.5, 0.999], [3.5, 3.5, 2.0001],
                    [5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [7.0, 5.0, 5.0]])  # exactly 1 apart, in the cells 4, 5 and 6: in
    want = _check(pn2, cuda, pts, 1.0, min_neighbors=1)
    assert want.count[[2, 4, 6, 8]].tolist() == [2, 2, 2, 2] and want.count[9:15].tolist() == [1] * 6
    assert want.count[15:].tolist() == [2, 3, 2]


# ---- beyond 65 536 points, by construction ---------------------------------------------------------------------------------------
def test_unit_lattice_by_construction(pn2, cuda):
    """a shuffled 42 x 42 x 40 unit lattice at radius 1: the neighbours of a point are itself and its axis partners, every one at
    distance exactly r.  Counts and moments come from array shifts, not from the model."""
    shape = (42, 42, 40)
    n = int(np.prod(shape))
    assert n > 65536
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    order = np.random.RandomState(0).permutation(n)
    pts = idx[order].astype(np.float32)
    got = _run(pn2, cuda, pts, None, 1.0, 3)
    Q, x, h = N.lattice(n, 1.0)
    assert (Q, x) == (20, 1) and got.header.tolist() == [0, n, n, 7, Q, x, 0, 0]
    unit = 1 << 19  # 1 / h
    want_count = np.ones(shape, dtype=np.int64)
    want_mom = np.zeros(shape + (9,), dtype=np.int64)
    for a, square in ((0, 3), (1, 6), (2, 8)):
        has_up = np.zeros(shape, dtype=np.int64)   # a partner at +1 along axis a
        has_down = np.zeros(shape, dtype=np.int64)
        up = [slice(None)] * 3
        up[a] = slice(0, shape[a] - 1)
        down = [slice(None)] * 3
        down[a] = slice(1, shape[a])
        has_up[tuple(up)] = 1
        has_down[tuple(down)] = 1
        want_count += has_up + has_down
        want_mom[..., a] = (has_up - has_down) * unit
        want_mom[..., square] = (has_up + has_down) * unit * unit
    assert np.array_equal(got.count, want_count.reshape(-1)[order].astype(np.int32))
    assert np.array_equal(got.moments, want_mom.reshape(-1, 9)[order])
    inside = ((idx[order] > 0) & (idx[order] < np.array(shape) - 1)).all(1)
    assert (got.count[inside] == 7).all() and inside.sum() == 40 * 40 * 38
    # an interior neighbourhood is isotropic: three equal eigenvalues, no rotation, the normal is the z axis
    assert (got.normals[inside] == [0.0, 0.0, 1.0]).all() and np.abs(got.curvature[inside] - 1.0 / 3.0).max() < 1e-7
    lam = np.float64(2 * unit * unit) / np.float64(7) * (h * h)
    assert (got.variance[inside] == lam).all() and not np.isnan(got.normals).any()


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(pn2, cuda):
    rs = np.random.RandomState(1)
    same = np.full((10, 3), [3.5, -2.25, 1e-3])
    want = _check(pn2, cuda, same, 0.5)
    assert want.count.tolist() == [10] * 10 and (want.moments == 0).all() and (want.variance == 0).all()
    assert (want.normals == [0.0, 0.0, 1.0]).all() and (want.curvature == 0).all()  # zero covariance: identity axes, 0 / 0 -> 0
    line = np.outer(np.arange(20) - 7.0, [0.5, 0.25, -1.0])
    want = _check(pn2, cuda, line, 3.0)
    assert (want.curvature < 1e-9).all() and want.count.max() == 5  # (a rounding residue of lambda_2 / trace at the most)
    one = np.array([[-7.0, 1e10, 3e-20]])
    assert _check(pn2, cuda, one, 2.0, min_neighbors=1).normals.tolist() == [[0.0, 0.0, 1.0]]
    want = _check(pn2, cuda, one, 2.0, min_neighbors=2)
    assert want.count.tolist() == [1] and np.isnan(want.normals).all() and want.header.tolist()[:4] == [0, 1, 0, 1]
    # groups of 1, 2, 3 and 4 points far from each other: count == min_neighbors - 1 and count == min_neighbors side by side
    groups = np.concatenate([rs.uniform(0, 0.3, (m, 3)) + [10.0 * m, 0, 0] for m in (1, 2, 3, 4)])
    want = _check(pn2, cuda, groups, 1.0, min_neighbors=3)
    assert want.count.tolist() == [1, 2, 2, 3, 3, 3, 4, 4, 4, 4] and np.isnan(want.normals[:3]).all() and not np.isnan(want.normals[3:]).any()
    assert (want.moments[1] != 0).any() and want.header[2] == 7
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, -0.0], [-0.0, 1.0, 0.0], [2.0, -0.0, -0.0], [-1.0, 0.0, -0.0]])
    _check(pn2, cuda, zeros, 1.5, min_neighbors=2)
    far = rs.random_sample((150, 3)) * [2.0, 2.0, 0.1] + [1e5, -1e5, 1e5]  # float32 steps of 1/128 at 10^5
    _check(pn2, cuda, far, 0.5)
    tiny = rs.randint(0, 6, (60, 3)) * 2.0 ** -149  # subnormal spacing and a subnormal radius
    _check(pn2, cuda, tiny, 3 * 2.0 ** -149, min_neighbors=2)
    huge = rs.uniform(-1, 1, (60, 3)) * 3e38
    _check(pn2, cuda, huge, 3e38, min_neighbors=2)


def test_invalid_points_between_members(pn2, cuda):
    rs = np.random.RandomState(2)
    n = BLOCK + 50
    pts = rs.uniform(0, 3, (n, 3)) * [1, 1, 0.2]
    labels = rs.randint(0, 4, n)
    labels[rs.choice(n, 40, replace=False)] = -1 - rs.randint(0, 5, 40)
    bad = rs.choice(n, 12, replace=False)
    pts[bad[:4], 0], pts[bad[4:8], 1], pts[bad[8:], 2] = np.nan, np.inf, -np.inf
    want = _check(pn2, cuda, pts, 0.6, labels)
    invalid = (labels < 0) | ~np.isfinite(pts.astype(np.float32)).all(1)
    assert (want.count[invalid] == 0).all() and (want.count[~invalid] >= 1).all() and (want.moments[invalid] == 0).all()
    assert np.isnan(want.normals[invalid]).all() and want.header[1] == (~invalid).sum()
    # every point invalid: nothing to scan
    want = _check(pn2, cuda, pts[:70], 0.6, np.full(70, -1))
    assert want.header.tolist() == [0, 0, 0, 0, N.lattice_bits(70), 0, 0, 0] and (want.count == 0).all()


def test_status_1_for_a_cloud_too_wide_for_the_grid(pn2, cuda):
    want = _check(pn2, cuda, np.array([[0, 0, 0], [1e7, 0, 0]]), 1.0, min_neighbors=1)
    assert want.header.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and want.count.tolist() == [0, 0] and (want.moments == 0).all()
    assert np.isnan(want.normals).all() and np.isnan(want.curvature).all() and np.isnan(want.variance).all()
    pts = np.random.RandomState(3).uniform(0, 1, (WAVE + 9, 3))
    pts[17, 1] = -3e6
    assert _check(pn2, cuda, pts, 1.0).header[0] == 1
    assert _check(pn2, cuda, np.array([[0, 0, 0], [2e6, 0, 0]]), 1.0, min_neighbors=1).header[0] == 0  # 2 * 10^6 cells: still fine


def test_neighbours_in_the_last_two_cells_of_every_axis(pn2, cuda):
    """the top edge of the grid: with radius = 1 and the minimum pinned at the origin, cell c of an axis is [c * h, (c + 1) * h),
    h = 1 + 2^-20, so 2097152.75 lies in cell 2^21 - 2 and 2097153.25 in cell 2^21 - 1, the last one (float32 resolves 0.25
    there); the diagonal pair is 0.5 * sqrt(3) apart: neighbours, found by a walk whose x range is clamped at the grid's edge
    (three points in three rows: the lane path)"""
    a, b = 2097152.75, 2097153.25
    pts = np.array([[0, 0, 0], [a, a, a], [b, b, b]], dtype=np.float32)
    cells = np.floor(pts.astype(np.float64) / (1.0 + 2.0 ** -20))
    assert (cells[1] == 2 ** 21 - 2).all() and (cells[2] == 2 ** 21 - 1).all()
    want = _check(pn2, cuda, pts, 1.0, min_neighbors=1)
    assert want.header[:4].tolist() == [0, 3, 3, 2] and want.count.tolist() == [1, 2, 2]


# ---- the viewpoint ---------------------------------------------------------------------------------------------------------------
def test_viewpoint(pn2, cuda):
    sheet = np.array([[x, y, 0] for x in range(3) for y in range(3)], dtype=np.float32)
    assert _check(pn2, cuda, sheet, 1.5, viewpoint=None).normals[4].tolist() == [0.0, 0.0, 1.0]
    assert _check(pn2, cuda, sheet, 1.5, viewpoint=(1, 1, 9)).normals[4].tolist() == [0.0, 0.0, 1.0]
    flipped = _check(pn2, cuda, sheet, 1.5, viewpoint=(1, 1, -2)).normals[4]
    assert flipped.tolist() == [0.0, 0.0, -1.0] and np.signbit(flipped).all()
    assert _check(pn2, cuda, sheet, 1.5, viewpoint=(7, 7, 0)).normals[4].tolist() == [0.0, 0.0, 1.0]  # w == 0 exactly: no flip
    rs = np.random.RandomState(4)
    ball = rs.standard_normal((300, 3))
    ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * 2.0 + [5.0, 5.0, 5.0]
    plain = _check(pn2, cuda, ball, 0.8)
    seen = _check(pn2, cuda, ball, 0.8, viewpoint=(5.0, 5.0, 5.0))  # from the centre: every normal points inwards
    full = ~np.isnan(plain.normals).any(1)
    assert full.sum() > 200 and ((seen.normals[full] * (ball[full] - 5.0)).sum(1) < 0).all()
    assert (np.abs(seen.normals[full]) == np.abs(plain.normals[full])).all() and (seen.normals[full] != plain.normals[full]).any()
    assert np.array_equal(seen.count, plain.count) and np.array_equal(seen.moments, plain.moments)


# ---- optional outputs, the order of the points -----------------------------------------------------------------------------------
def test_optional_outputs_and_permutation(pn2, cuda):
    rs = np.random.RandomState(5)
    n = BLOCK + 77
    pts = np.ascontiguousarray(rs.uniform(0, 2.5, (n, 3)) * [1, 1, 0.25], dtype=np.float32)
    labels = np.where(rs.random_sample(n) < 0.1, -1, 0).astype(np.int32)
    full = _run(pn2, cuda, pts, labels, 0.5, 3, (0.0, 0.0, 10.0))
    for moments, variance in ((False, False), (True, False), (False, True)):
        part = _run(pn2, cuda, pts, labels, 0.5, 3, (0.0, 0.0, 10.0), moments=moments, variance=variance)
        assert (part.moments is None) == (not moments) and (part.variance is None) == (not variance)
        for name in ("count", "normals", "curvature", "header") + (("moments",) if moments else ()) + (("variance",) if variance else ()):
            assert getattr(part, name).tobytes() == getattr(full, name).tobytes(), name
    # a shuffled copy gives the permuted outputs (device against device; `full` against the model once)
    order = rs.permutation(n)
    other = _run(pn2, cuda, np.ascontiguousarray(pts[order]), np.ascontiguousarray(labels[order]), 0.5, 3, (0.0, 0.0, 10.0))
    for name in ("count", "moments", "normals", "curvature", "variance"):
        assert getattr(other, name).tobytes() == np.ascontiguousarray(getattr(full, name)[order]).tobytes(), name
    assert other.header.tolist() == full.header.tolist()
    _check(pn2, cuda, pts, 0.5, labels, 3, (0.0, 0.0, 10.0))


# ---- refusals that need a device -------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(pn2, cuda):
    import torch
    lib = pn2._lib
    n = 100
    pts = torch.zeros((n, 3), dtype=torch.float32, device=cuda)
    outs = [_guarded(torch, cuda, b) for b in (4 * n, 72 * n, 12 * n, 4 * n, 24 * n, 32)]
    (count, mom, nrm, curv, var, hdr) = [o[1] for o in outs]
    nbytes = ctypes.c_ulonglong(0)
    lib.launch("pn2_radius_workspace_size", cuda, n, ctypes.byref(nbytes), stream=False)
    need = int(nbytes.value)
    ws = torch.full((need + 512,), POISON, dtype=torch.uint8, device=cuda)
    off = (-ws.data_ptr()) % 256

    def call(n=n, radius=0.5, min_neighbors=3, view=None, workspace=ws.data_ptr() + off, nbytes=need, count=count):
        return lib.lib.pn2_radius_neighborhoods(n, lib.ptr(pts), None, radius, min_neighbors, view, lib.ptr(count), lib.ptr(mom),
                                                lib.ptr(nrm), lib.ptr(curv), lib.ptr(var), lib.ptr(hdr), workspace, nbytes,
                                                lib.stream_ptr())
    assert call(nbytes=need - 1) == -1 and call(nbytes=16) == -1 and call(workspace=ws.data_ptr() + off + 128) == -1
    assert call(min_neighbors=0) == -1 and call(radius=float("nan")) == -1 and call(n=0) == -1
    assert call(view=_view((0.0, float("inf"), 0.0))) == -1 and call(count=None) == -2
    torch.cuda.synchronize()
    assert all((o[0] == POISON).all() for o in outs) and (ws == POISON).all()
    assert call() == 0  # the same buffers, accepted
    torch.cuda.synchronize()
    assert _payload(outs[0][0], 4 * n, "count").view(np.int32).tolist() == [n] * n


# ---- the wrappers, the KITTI method, the example ---------------------------------------------------------------------------------
def test_wrappers_and_kitti_method(pn2, cuda):
    import torch
    rs = np.random.RandomState(6)
    n = 300
    pts64 = rs.uniform(0, 3, (n, 3)) * [1, 1, 0.1] + [4.0, -2.0, 1.0]
    pts32 = pts64.astype(np.float32)
    labels = rs.randint(-1, 4, n)
    d_pts = torch.from_numpy(pts32).to(cuda)

    def same(nb, want, moments, variance):
        assert isinstance(nb, pn2.Neighborhoods) and all(t.device == cuda for t in nb[:3])
        assert (nb.status, nb.valid, nb.lattice) == (int(want.header[0]), int(want.header[1]), (int(want.header[4]), int(want.header[5])))
        assert nb.count.dtype == torch.int32 and nb.normals.dtype == torch.float32 and nb.curvature.dtype == torch.float32
        assert nb.count.cpu().numpy().tobytes() == want.count.tobytes() and nb.normals.cpu().numpy().tobytes() == want.normals.tobytes()
        assert nb.curvature.cpu().numpy().tobytes() == want.curvature.tobytes()
        assert (nb.moments is None) == (not moments) and (nb.variance is None) == (not variance)
        if moments:
            assert nb.moments.dtype == torch.int64 and np.array_equal(nb.moments.cpu().numpy(), want.moments)
        if variance:
            assert nb.variance.dtype == torch.float64 and nb.variance.cpu().numpy().tobytes() == want.variance.tobytes()

    plain = N.neighborhoods(pts32, 0.5, None, 3, None)
    same(pn2.radius_neighborhoods(d_pts, 0.5), plain, False, False)
    same(pn2.radius_neighborhoods(pts64, np.float64(0.5), moments=True, variance=True), plain, True, True)  # numpy, float64: cast
    lab = N.neighborhoods(pts32, 0.5, labels, 4, (0.0, 0.0, 0.0))
    same(pn2.radius_neighborhoods(d_pts, 0.5, labels=torch.from_numpy(labels).to(cuda), min_neighbors=4, viewpoint=(0, 0, 0),
                                  moments=True), lab, True, False)
    only = N.neighborhoods(pts32, 0.5, np.where(np.isin(labels, [1, 3]), labels, -1), 3, None)
    same(pn2.radius_neighborhoods(pts32, 0.5, labels=labels, classes=[3, 1], variance=True), only, False, True)
    normals = pn2.estimate_normals(d_pts, 0.5)
    assert normals.cpu().numpy().tobytes() == plain.normals.tobytes()
    toward = N.neighborhoods(pts32, 0.5, None, 5, (0.0, 0.0, 0.0))
    assert pn2.estimate_normals(d_pts, 0.5, viewpoint=(0, 0, 0), min_neighbors=5).cpu().numpy().tobytes() == toward.normals.tobytes()
    frame = types.SimpleNamespace(points=d_pts)
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)  # the method uses none of the network's state
    assert predictor.normals_for_frame(frame, 0.5, min_neighbors=5).cpu().numpy().tobytes() == toward.normals.tobytes()
    assert torch.equal(predictor.normals_for_frame(frame, 0.5), pn2.estimate_normals(d_pts, 0.5, viewpoint=(0, 0, 0)))
    indices, mask = pn2.remove_radius_outlier(d_pts, 6, 0.5, labels=labels)
    want = N.neighborhoods(pts32, 0.5, labels, 6, None).count >= 6
    assert indices.dtype == torch.int64 and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want)
    assert indices.tolist() == np.nonzero(want)[0].tolist()
    colors = pn2.normal_colors(normals)
    bad = np.isnan(plain.normals).any(1, keepdims=True)
    want_rgb = np.where(bad, 96, np.rint((np.where(bad, 0, plain.normals) * np.float32(0.5) + np.float32(0.5)) * np.float32(255))).astype(np.uint8)
    assert colors.device == cuda and np.array_equal(colors.cpu().numpy(), want_rgb)
    image = pn2.render.render_colors(d_pts, colors, "top", width=160, height=120)
    assert tuple(image.shape) == (120, 160, 3)
    # nothing to look at, and a cloud too wide for the grid
    none = pn2.radius_neighborhoods(d_pts[:0], 0.5, moments=True)
    assert none.count.shape == (0,) and none.normals.shape == (0, 3) and none.moments.shape == (0, 9) and none.valid == 0
    wide = torch.tensor([[0.0, 0, 0], [1e7, 0, 0]], device=cuda)
    assert pn2.radius_neighborhoods(wide, 1.0).status == 1
    with pytest.raises(ValueError, match="2\\^21 cells"):
        pn2.estimate_normals(wide, 1.0)
    with pytest.raises(ValueError, match="2\\^21 cells"):
        pn2.remove_radius_outlier(wide, 2, 1.0)


def test_remove_radius_outlier_on_a_planted_case(pn2, cuda):
    """a 2000-point slab plus 40 isolated points: exactly those are removed"""
    rs = np.random.RandomState(7)
    slab = rs.uniform(0, 1, (2000, 3)) * [10.0, 10.0, 0.2]   # 20 points per unit square: about 15 within 0.5 of a point
    stray = np.stack([np.arange(40) % 8 * 1.5, np.arange(40) // 8 * 1.5, np.full(40, 3.0)], 1)  # 1.5 apart, 2.8 above the slab
    pts = np.concatenate([slab, stray]).astype(np.float32)
    order = rs.permutation(len(pts))
    pts = pts[order]
    planted = order >= 2000
    indices, mask = pn2.remove_radius_outlier(pts, 2, 0.5)
    assert np.array_equal(mask.cpu().numpy(), ~planted) and indices.tolist() == np.nonzero(~planted)[0].tolist()
    nb = pn2.radius_neighborhoods(pts, 0.5, min_neighbors=2)
    assert (nb.count.cpu().numpy()[planted] == 1).all() and nb.valid == 2040 and nb.status == 0
    assert np.isnan(nb.normals.cpu().numpy()[planted]).all() and not np.isnan(nb.normals.cpu().numpy()[~planted]).any()


def test_example(pn2, cuda, tmp_path):
    n = 3000
    out = str(tmp_path / "normals")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "estimate_normals.py"), "--synthetic", str(n), "--out", out,
                          "--width", "320", "--height", "200"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    spec = importlib.util.spec_from_file_location("estimate_normals_example", os.path.join(ROOT, "examples", "estimate_normals.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    pts, planted = example.synthetic(n)
    assert len(pts) == n and planted.sum() == n // 50
    with open(os.path.join(out, "outliers.txt")) as f:
        assert [int(line) for line in f.read().split()] == np.nonzero(planted)[0].tolist()
    with open(os.path.join(out, "normals.png"), "rb") as f:
        png = f.read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", png[16:24]) == (320, 200)
