"""CPU tests of fixed-radius neighbourhoods (csrc/pn2_neighbors.hip, neighbors.py): the numpy model of the rules
(tests/neighbors_ref.py) against independent code -- scipy's KD-tree for the counts, np.cov / np.linalg.eigh for the spectrum and
the axes --, the properties the rules promise (exactly diagonal after eight sweeps, |q| <= 2^Q, sums far below 2^63), the header's
prototypes, every refusal of the entry point that needs no GPU and their order, the wrapper's argument errors and its refusal of
a capturing stream, and the two helpers that are plain torch ops.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import describe_ref as D  # noqa: E402
import neighbors_ref as N  # noqa: E402

ARGS = {
    "pn2_radius_workspace_size": ("n", "bytes"),
    "pn2_radius_neighborhoods": ("n", "points", "labels", "radius", "min_neighbors", "viewpoint", "count", "moments", "normals",
                                 "curvature", "variance", "header", "workspace", "workspace_bytes", "stream"),
}


def _noisy_plane(seed, n=1500):
    """n points on a tilted 6 x 6 sheet with 0.02 of noise across it"""
    rs = np.random.RandomState(seed)
    uv = rs.uniform(-3, 3, (n, 2))
    z = 0.3 * uv[:, 0] - 0.2 * uv[:, 1] + rs.normal(0, 0.02, n)
    return np.stack([uv[:, 0], uv[:, 1], z], 1).astype(np.float32)


def _blobs(seed, n=400):
    """a line, a sheet and a ball next to each other, offset from the origin"""
    rs = np.random.RandomState(seed)
    k = n // 4
    line = np.outer(rs.uniform(-1, 1, k), [1.0, 0.5, 0.25])
    sheet = np.concatenate([rs.uniform(-1, 1, (k, 2)), np.zeros((k, 1))], 1) + [3, 0, 0]
    ball = rs.standard_normal((n - 2 * k, 3)) * 0.4 + [0, 3, 0]
    return (np.concatenate([line, sheet, ball]) + [100.0, -50.0, 7.0]).astype(np.float32)


# ---- the model against independent code ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,radius,with_labels", [(0, 0.4, False), (1, 0.25, True), (2, 1.0, False)])
def test_model_counts_against_a_kd_tree(seed, radius, with_labels):
    spatial = pytest.importorskip("scipy.spatial")
    pts = _noisy_plane(seed)
    labels = np.random.RandomState(seed).randint(-1, 3, len(pts)).astype(np.int32) if with_labels else None
    pts[5] = [np.nan, 0, 0]
    out = N.neighborhoods(pts, radius, labels, min_neighbors=10 ** 9)  # counts only: no point reaches the eigen stage
    ok = N.valid_mask(pts, labels)
    at = np.nonzero(ok)[0]
    tree = spatial.cKDTree(pts[at].astype(np.float64))
    want = np.zeros(len(pts), dtype=np.int32)
    want[at] = [len(v) for v in tree.query_ball_point(pts[at].astype(np.float64), float(np.float32(radius)))]
    assert np.array_equal(out.count, want)
    assert out.count[at].min() >= 1 and out.count[~ok].max() == 0 and out.header[1] == ok.sum() and out.header[3] == want.max()
    assert out.header[2] == 0 and np.isnan(out.normals).all() and (out.moments[~ok] == 0).all()


@pytest.mark.parametrize("seed,radius", [(0, 0.4), (3, 0.7), (4, 0.05)])
def test_model_against_cov_and_eigh(seed, radius):
    """The bound is derived, not fitted, as in test_describe_cpu.py with E = 2 r: the neighbours' differences u lie in [-r, r]
    per axis, an interval of length E = 2 r, and snapping to the lattice moves each by du, |du| <= h / 2.  An entry of the
    covariance moves by Cov(u, dv) + Cov(du, v) + Cov(du, dv); |Cov(u, dv)| = |E[(u - mean u) dv]| <= E * h / 2, and
    |Cov(du, dv)| = |E[(du - mean du) dv]| <= h * h / 2, so an entry moves by at most E * h + h^2 / 2.  The eigenvalues of a
    symmetric 3 x 3 matrix move by at most the spectral norm of the perturbation, <= 3 * (E * h + h^2 / 2) < 4 * E * h, because
    h <= E * 2^-14.  Float64 noise of np.cov and eigvalsh: a few ulps of E^2; 1e-12 * E^2 is four orders above that."""
    pts = _noisy_plane(seed, 300) if seed != 4 else (_noisy_plane(seed, 300) * 0.1 + 1000.0).astype(np.float32)
    n = len(pts)
    r = float(np.float32(radius))
    out = N.neighborhoods(pts, radius, None, 3, viewpoint=None)
    Q, x, h = N.lattice(n, radius)
    assert (out.header[4], out.header[5]) == (Q, x) and 0.5 <= r / 2.0 ** x < 1.0 and h == 2.0 ** (x - Q)
    E = 2.0 * r
    bound = 4.0 * E * h + 1e-12 * E * E
    p64 = pts.astype(np.float64)
    checked = 0
    for i, d in N.neighbour_rows(p64, np.ones(n, dtype=bool), radius):
        if len(d) < 3:
            assert np.isnan(out.normals[i]).all() and np.isnan(out.curvature[i]) and np.isnan(out.variance[i]).all()
            continue
        cov = np.cov(d.T, bias=True)
        want = np.linalg.eigvalsh(cov)[::-1]
        assert np.abs(out.variance[i] - want).max() <= bound, (i, out.variance[i], want, bound)
        # the axes the normal is taken from: orthonormal, right-handed, and they diagonalise np.cov to the same bound
        q = np.rint(d / h).astype(np.int64)
        _, A = D.covariance(N.moments_of(q), len(q))
        _, a0, a1, a2, _ = D.axes_of(A, 0)
        R = np.stack([a0, a1, a2])
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
        off = R @ cov @ R.T
        assert np.abs(off - np.diag(np.diag(off))).max() <= bound
        # the normal is +-a2 rounded once to float32, its largest component positive without a viewpoint
        nrm = out.normals[i].astype(np.float64)
        assert np.abs(nrm - D.fix_sign(a2)).max() <= 2.0 ** -24 and nrm[np.argmax(np.abs(nrm))] > 0
        # curvature: lambda_2 / trace.  lambda_2 is off by <= bound, the trace by <= 3 * bound, and c <= 1/3: the quotient is
        # off by <= 2 * bound / (trace - 3 * bound) <= 3 * bound / trace once trace >= 9 * bound; 2^-23 covers the float32 rounding
        tr = want.sum()
        if tr > 1e3 * bound:
            assert abs(float(out.curvature[i]) - want[2] / tr) <= 3.0 * bound / tr + 2.0 ** -23
        assert 0.0 <= out.curvature[i] <= 1.0 / 3.0 + 2.0 ** -23
        checked += 1
    assert checked > 100


def test_off_diagonals_are_exactly_zero_after_eight_sweeps():
    """on the covariances the neighbourhoods of a cloud give (lines, sheets, balls and the edges between them), not on random
    matrices: after the eight sweeps the three off-diagonal entries are exactly 0.0"""
    for pts, radius in ((_blobs(0), 0.5), (_noisy_plane(1, 400), 0.6)):
        n = len(pts)
        _, _, h = N.lattice(n, radius)
        for i, d in N.neighbour_rows(pts.astype(np.float64), np.ones(n, dtype=bool), radius):
            q = np.rint(d / h).astype(np.int64)
            _, A = D.covariance(N.moments_of(q), len(q))
            after = D.axes_of(A, 0)[4]
            assert after[0, 1] == 0.0 and after[0, 2] == 0.0 and after[1, 2] == 0.0, (i, after)


def test_lattice_coordinates_and_sums_stay_in_range():
    for bitlen in range(1, 32):
        for n in {1 << (bitlen - 1), (1 << bitlen) - 1}:
            Q = N.lattice_bits(n)
            assert 14 <= Q <= 20 and n * (1 << Q) ** 2 <= 2 ** 60 < 2 ** 62, n
    assert N.lattice_bits(2 ** 31 - 1) == 14 and N.lattice_bits(2 ** 20 - 1) == 20 and N.lattice_bits(2 ** 20) == 19
    # the largest difference the test lets through, r * (1 + 2^-51), at both ends of f and of the exponent range
    one_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    for radius in (np.float32(0.5), one_below, np.float32(3.0e38), np.float32(1e-45), np.float32(0.4), np.float32(5.0)):
        for n in (1, 2 ** 20, 2 ** 31 - 1):
            Q, x, h = N.lattice(n, radius)
            r = np.float64(radius)
            assert 0.5 <= r / 2.0 ** x < 1.0
            dmax = r * (1.0 + 2.0 ** -51)
            q = int(np.rint(dmax / h))
            assert q <= 1 << Q and int(np.rint(-dmax / h)) == -q, (radius, n)
            assert (dmax / h) * h == dmax  # the division by a power of two is exact
    # every neighbour at the far corner of the lattice, n = 2^22 of them
    Q = N.lattice_bits(2 ** 22)
    S = N.moments_of(np.full((1, 3), 1 << Q, dtype=np.int64))
    assert Q == 18 and all(v * 2 ** 22 < 2 ** 62 for v in S) and S[3] * 2 ** 22 == 2 ** 58


def test_model_hand_made_cases():
    # the point itself counts; <= at the boundary; the partner one float32 step further is out
    pts = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 5], [9, 9, 9]], dtype=np.float32)
    out = N.neighborhoods(pts, 5.0, None, 1)
    assert out.count.tolist() == [3, 2, 2, 1] and out.header.tolist() == [0, 4, 4, 3, 20, 3, 0, 0]
    h = 2.0 ** (3 - 20)
    assert out.moments[0].tolist() == [int(3 / h), int(4 / h), int(5 / h), int(9 / h / h), int(12 / h / h), 0, int(16 / h / h), 0, int(25 / h / h)]
    assert N.neighborhoods(pts, np.nextafter(np.float32(5.0), np.float32(0.0)), None, 1).count.tolist() == [1, 1, 1, 1]
    # a single point: zero covariance, identity axes, normal (0,0,1), curvature 0 / 0 -> 0
    assert out.normals[3].tolist() == [0.0, 0.0, 1.0] and out.curvature[3] == 0.0 and out.variance[3].tolist() == [0.0] * 3
    # min_neighbors: count and moments kept, NaNs
    out2 = N.neighborhoods(pts, 5.0, None, 3)
    assert out2.count.tolist() == [3, 2, 2, 1] and np.array_equal(out2.moments, out.moments) and out2.header[2] == 1
    assert np.isnan(out2.normals[1:]).all() and not np.isnan(out2.normals[0]).any() and np.isnan(out2.curvature[1:]).all()
    # a viewpoint below the sheet z = 0 turns the normal down; w == 0 (a viewpoint in the sheet) and NaN change nothing
    sheet = np.array([[x, y, 0] for x in range(3) for y in range(3)], dtype=np.float32)
    assert N.neighborhoods(sheet, 1.5, None, 3).normals[4].tolist() == [0.0, 0.0, 1.0]
    assert N.neighborhoods(sheet, 1.5, None, 3, viewpoint=(1, 1, -2)).normals[4].tolist() == [-0.0, -0.0, -1.0]
    assert N.neighborhoods(sheet, 1.5, None, 3, viewpoint=(7, 7, 0)).normals[4].tolist() == [0.0, 0.0, 1.0]
    # invalid points: non-finite rows and negative labels are nobody's neighbours
    pts = np.array([[0, 0, 0], [np.inf, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    out = N.neighborhoods(pts, 2.0, np.array([0, 0, -1, 5]), 1)
    assert out.count.tolist() == [2, 0, 0, 2] and out.header[1] == 2 and np.isnan(out.normals[[1, 2]]).all()
    # status 1
    out = N.neighborhoods(np.array([[0, 0, 0], [1e7, 0, 0]], dtype=np.float32), 1.0, None, 1)
    assert out.header.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and out.count.tolist() == [0, 0] and np.isnan(out.normals).all()
    assert N.neighborhoods(np.array([[0, 0, 0], [2e6, 0, 0]], dtype=np.float32), 1.0, None, 1).header[0] == 0


def test_models_place_a_pair_in_the_last_two_cells():
    """the input of the GPU tests of the grid's top edge: with an edge of 1 * (1 + 2^-20) and the minimum at the origin,
    2097152.75 is in cell 2^21 - 2 and 2097153.25 in cell 2^21 - 1 on every axis; both models accept the cloud (status 0) and
    link the pair"""
    import cluster_ref as C
    a, b = 2097152.75, 2097153.25
    pts = np.array([[0, 0, 0], [a, a, a], [b, b, b]], dtype=np.float32)
    assert pts[1, 0] == a and pts[2, 0] == b  # float32 resolves 0.25 there
    cells = np.floor(pts.astype(np.float64) / (1.0 + 2.0 ** -20))
    assert (cells[1] == 2 ** 21 - 2).all() and (cells[2] == 2 ** 21 - 1).all()
    out = N.neighborhoods(pts, 1.0, None, 1)
    assert out.header[:4].tolist() == [0, 3, 3, 2] and out.count.tolist() == [1, 2, 2]
    ids, hdr = C.cluster(pts, 1.0, None, 1, 0)
    assert ids.tolist() == [0, 1, 1] and hdr.tolist() == [0, 2, 2, 3, 3, 0, 0, 0]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS and name not in pn2._lib._STATEFUL
    i, f, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_radius_workspace_size"].argtypes == [i, p]
    assert fns["pn2_radius_neighborhoods"].argtypes == [i, p, p, f, i, p, p, p, p, p, p, p, p, z, p]
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_neighbors.hip" in pn2._lib._build.SOURCES
    csrc = os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc")
    for name in ("pn2_neighbors.hip", "pn2_cell_grid.h", "pn2_eig3.h"):
        with open(os.path.join(csrc, name)) as src:
            assert "pn2_grid_knn.h" not in src.read(), name
    # the shared pieces exist once
    for name, owner in (("grid_min_kernel(", "pn2_cell_grid.h"), ("grid_key_kernel(", "pn2_cell_grid.h"),
                        ("grid_gather_kernel(", "pn2_cell_grid.h"), ("lower_bound_key(const", "pn2_cell_grid.h"),
                        ("void grid_walk_rows(", "pn2_cell_grid.h"), ("unsigned long long row_key(", "pn2_cell_grid.h"),
                        ("bool cell_in(", "pn2_cell_grid.h"), ("Cell key_cell(", "pn2_cell_grid.h"),
                        ("void grid_scal_reset(", "pn2_cell_grid.h"), ("struct CellGrid", "pn2_cell_grid.h"),
                        ("void jacobi_rotate(", "pn2_eig3.h"), ("void fix_sign(", "pn2_eig3.h")):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and name in open(os.path.join(csrc, f)).read()]
        assert holders == [owner], (name, holders)
    # no grid kernel is launched, and no row searched, outside the grid's header -- but for the wave-uniform path's own search
    # and clustering's written-out walk in front of a point
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            text = open(os.path.join(csrc, f)).read()
            assert not any("grid_%s_kernel<<<" % k in text for k in ("min", "key", "gather")), f
            assert text.count("lower_bound_key(") == (1 if f in ("pn2_neighbors.hip", "pn2_cluster.hip") else 0), f
    for name in ("radius_neighborhoods", "estimate_normals", "remove_radius_outlier", "normal_colors", "Neighborhoods"):
        assert getattr(pn2, name) is getattr(pn2.neighbors, name), name
    assert pn2.Neighborhoods._fields == ("count", "normals", "curvature", "variance", "moments", "lattice", "valid", "status")
    assert callable(pn2.kitti_predict.PredictInterpolator.normals_for_frame)


def _workspace_bytes(pn2, n):
    nbytes = ctypes.c_ulonglong(0)
    assert pn2._lib.lib.pn2_radius_workspace_size(n, ctypes.byref(nbytes)) == 0
    return int(nbytes.value)


def test_workspace_size(pn2):
    K = pn2._lib.ABI.constants
    query = pn2._lib.lib.pn2_radius_workspace_size
    nbytes = ctypes.c_ulonglong(7)
    assert query(0, ctypes.byref(nbytes)) == K["PN2_EINVAL"] and query(-4, ctypes.byref(nbytes)) == K["PN2_EINVAL"]
    assert query(100, None) == K["PN2_ENULL"] and nbytes.value == 7
    size = lambda n: _workspace_bytes(pn2, n)  # noqa: E731
    # per point: two keys, two indices and one (x, y, z, -) row; the scalars and the sort's own storage on top
    assert size(1) % 256 == 0 and size(1000) >= 1000 * (2 * 8 + 2 * 4 + 16) and size(1000) <= size(1001)


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL = K["PN2_EINVAL"], K["PN2_ENULL"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    view = lambda *v: (ctypes.c_double * 3)(*v)  # noqa: E731  (the viewpoint is host memory and IS read)
    n = 1000
    need = _workspace_bytes(pn2, n)
    names = pn2._lib.ABI.functions["pn2_radius_neighborhoods"].argnames
    # the good call would reach the stream query: every call below differs from it in at least one refused argument
    good = dict(n=n, points=fake, labels=fake, radius=0.5, min_neighbors=3, viewpoint=view(0, 0, 0), count=fake, moments=fake,
                normals=fake, curvature=fake, variance=fake, header=fake, workspace=fake, workspace_bytes=need, stream=None)

    def call(**change):
        a = dict(good, **change)
        return pn2._lib.lib.pn2_radius_neighborhoods(*[a[k] for k in names])

    for bad in (dict(n=0), dict(n=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
                dict(min_neighbors=0), dict(min_neighbors=-2), dict(viewpoint=view(float("nan"), 0, 0)),
                dict(viewpoint=view(0, float("inf"), 0)), dict(viewpoint=view(0, 0, float("-inf")))):
        assert call(**bad) == EINVAL, bad
    for required in ("points", "count", "normals", "curvature", "header", "workspace"):
        assert call(**{required: None}) == ENULL, required
    for k in ("points", "labels", "count", "normals", "curvature", "header"):
        assert call(**{k: odd(2)}) == EINVAL, k
    for k in ("moments", "variance"):
        assert call(**{k: odd(4)}) == EINVAL, k
    assert call(workspace=odd(128)) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    # optional arguments may be NULL: what remains wrong is still what is reported
    assert call(labels=None, moments=None, variance=None, viewpoint=None, workspace_bytes=0) == EINVAL
    assert call(labels=None, moments=None, variance=None, viewpoint=None, header=None) == ENULL
    # the order: values (the viewpoint among them), NULL, alignment and workspace
    assert call(radius=0.0, points=None) == EINVAL and call(viewpoint=view(float("nan"), 0, 0), count=None) == EINVAL
    assert call(min_neighbors=0, workspace=odd(128)) == EINVAL
    assert call(header=None, workspace_bytes=0) == ENULL and call(curvature=None, moments=odd(4)) == ENULL
    assert call(normals=None, points=odd(2)) == ENULL


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def _library_must_not_be_reached(pn2, monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pn2.neighbors, "launch", fail)
    monkeypatch.setattr(pn2.cluster, "_on_device", fail)
    monkeypatch.setattr(pn2.cluster, "_device_of", fail)


def test_wrapper_argument_errors(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)  # (torch's own asks for a device)
    pts = np.zeros((10, 3), dtype=np.float32)
    rn = pn2.radius_neighborhoods
    for bad in (np.zeros((10, 4), dtype=np.float32), np.zeros((10,), dtype=np.float32), np.zeros((2, 5, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="points"):
            rn(bad, 0.5)
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1e39, "wide", None):
        with pytest.raises(ValueError, match="radius"):
            rn(pts, radius)
        with pytest.raises(ValueError, match="radius"):
            pn2.estimate_normals(pts, radius)
        with pytest.raises(ValueError, match="radius"):
            pn2.remove_radius_outlier(pts, 3, radius)
    for m in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="min_neighbors"):
            rn(pts, 0.5, min_neighbors=m)
        with pytest.raises(ValueError, match="nb_points"):
            pn2.remove_radius_outlier(pts, m, 0.5)
    for v in ((0, 0), (0, 0, 0, 0), (0, float("nan"), 0), (float("inf"), 0, 0), 3.0, ("a", "b", "c")):
        with pytest.raises(ValueError, match="viewpoint"):
            rn(pts, 0.5, viewpoint=v)
    with pytest.raises(ValueError, match="labels"):
        rn(pts, 0.5, labels=np.zeros(9, dtype=np.int32))
    with pytest.raises(ValueError, match="labels: integers"):
        rn(pts, 0.5, labels=np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError, match="classes"):
        rn(pts, 0.5, classes=[1])
    with pytest.raises(ValueError, match="classes"):
        rn(pts, 0.5, labels=np.zeros(10, dtype=np.int32), classes=[-1])
    for bad in (np.zeros((4, 3)), torch.zeros((4, 2)), torch.zeros((4, 3), dtype=torch.int32), torch.zeros((3,))):
        with pytest.raises(ValueError, match="normals"):
            pn2.normal_colors(bad)


def test_wrapper_refuses_a_capturing_stream(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    pts = np.zeros((10, 3), dtype=np.float32)
    for call in (lambda p, r: pn2.radius_neighborhoods(p, r), lambda p, r: pn2.estimate_normals(p, r),
                 lambda p, r: pn2.remove_radius_outlier(p, 3, r)):
        with pytest.raises(RuntimeError, match="capturing"):
            call(pts, 0.5)
        with pytest.raises(RuntimeError, match="capturing"):  # before the arguments are looked at
            call(np.zeros((10, 4), dtype=np.float32), -1.0)
    frame = type("Frame", (), {"points": pts})()
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)
    with pytest.raises(RuntimeError, match="capturing"):
        predictor.normals_for_frame(frame, 0.5)


def test_normal_colors_and_the_outlier_selection_on_host_tensors(pn2):
    import torch
    nan = float("nan")
    normals = torch.tensor([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.25, -0.5, 0.75], [nan, nan, nan], [0.0, nan, 1.0],
                            [1.0 / 255.0, -1.0 / 255.0, 3.0 / 255.0]], dtype=torch.float32)
    rgb = pn2.normal_colors(normals)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (6, 3)
    want = np.rint((normals.numpy().astype(np.float64) * 0.5 + 0.5) * 255)
    want[[3, 4]] = 96
    # (every product and sum of these rows is exact in float32 but the last row's, which is nowhere near a tie)
    assert rgb.tolist() == want.astype(np.uint8).tolist()
    assert rgb[0].tolist() == [128, 128, 255] and rgb[1].tolist() == [0, 128, 128] and rgb[3].tolist() == [96, 96, 96]
    assert rgb[5].tolist() == [128, 127, 129]  # 128.0, 127.0, 129.0: whole numbers
    assert pn2.normal_colors(normals.double()).tolist() == rgb.tolist()
    assert tuple(pn2.normal_colors(torch.zeros((0, 3))).shape) == (0, 3)
    count = torch.tensor([0, 3, 1, 5, 2, 3, 0], dtype=torch.int32)
    indices, mask = pn2.neighbors.select_by_count(count, 3)
    assert indices.tolist() == [1, 3, 5] and indices.dtype == torch.int64 and mask.tolist() == [False, True, False, True, False, True, False]
    indices, mask = pn2.neighbors.select_by_count(count, 1)  # count >= 1: the valid points
    assert indices.tolist() == [1, 2, 3, 4, 5] and mask.dtype == torch.bool
    assert pn2.neighbors.select_by_count(count, 6)[0].tolist() == []
