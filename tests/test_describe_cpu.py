"""CPU tests of object description: the numpy model (tests/describe_ref.py) against np.cov / np.linalg.eigvalsh, the properties the
rules promise (exactly diagonal after eight sweeps, moments below 2^62), the header, and every refusal that needs no GPU -- the
library's argument checks and the wrapper's."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import describe_ref as D  # noqa: E402

ARGS = {
    "pn2_cluster_describe_workspace_size": ("nclusters", "bytes"),
    "pn2_cluster_describe": ("n", "nclusters", "points", "ids", "upright", "moments", "desc", "workspace", "workspace_bytes", "stream"),
    "pn2_box_wireframe": ("nclusters", "desc", "per_edge", "points", "owner", "stream"),
}


def _rotation(rs):
    q, r = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _cloud(rs, m, offset):
    """m points, normal with standard deviations 3 : 1 : 0.2 (times a random scale), turned by a random rotation"""
    scale = 10.0 ** rs.uniform(-2, 2)
    return ((rs.standard_normal((m, 3)) * [3.0, 1.0, 0.2] * scale) @ _rotation(rs).T + offset).astype(np.float32)


# ---- the model against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_model_against_cov_and_eigvalsh(seed):
    """The bound is derived, not fitted: snapping to the lattice moves a coordinate by at most h / 2, so a centred second moment
    E[(u + du)(v + dv)] moves by at most 2 * (E / 2) * (h / 2) * 2 + h^2 / 4 < E * h (|u|, |v| <= E about any point of the box,
    the mean shifts by at most h / 2 as well), and the eigenvalues of a symmetric matrix move by at most the spectral norm of the
    perturbation, <= 3 * E * h for a 3 x 3 matrix with entries below E * h: 4 * E * h covers it.  Float64 noise: np.cov centres
    first, so its entries and eigvalsh carry a few ulps of E^2: 1e-12 * E^2 is four orders above that and six below 4 * E * h."""
    rs = np.random.RandomState(seed)
    m = int(rs.choice([5, 64, 1000, 5000]))
    pts = _cloud(rs, m, rs.uniform(-50, 50, 3) if seed % 2 else np.zeros(3))
    moments, desc = D.describe(pts, np.zeros(m, dtype=np.int32), 1, 0)
    p64 = pts.astype(np.float64)
    E = (p64.max(0) - p64.min(0)).max()
    Q, x = int(moments[0, 10]), int(moments[0, 11])
    h = 2.0 ** (x - Q)
    assert 0.5 <= E / 2.0 ** x < 1.0 and Q == D.lattice_bits(m) and moments[0, 0] == m
    want = np.linalg.eigvalsh(np.cov(p64.T, bias=True))[::-1]
    bound = 4.0 * E * h + 1e-12 * E * E
    assert np.abs(desc[0, 3:6] - want).max() <= bound, (np.abs(desc[0, 3:6] - want).max(), bound)
    assert np.abs(desc[0, 0:3] - p64.mean(0)).max() <= h  # the centroid: every coordinate moved by at most h / 2
    # the axes: orthonormal, right-handed, and they diagonalise the covariance to the same bound
    R = desc[0, 6:15].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    off = R @ np.cov(p64.T, bias=True) @ R.T
    assert np.abs(off - np.diag(np.diag(off))).max() <= bound
    # the box holds every member: lo <= a_k . (p - centroid) <= hi, and the centre is its middle
    t = (p64 - desc[0, 0:3]) @ R.T
    assert (t >= desc[0, 15:18] - 1e-9 * E).all() and (t <= desc[0, 18:21] + 1e-9 * E).all()
    mid = desc[0, 0:3] + (0.5 * (desc[0, 15:18] + desc[0, 18:21])) @ R
    assert np.abs(mid - desc[0, 21:24]).max() <= 1e-12 * (E + np.abs(p64).max())


def test_model_upright_keeps_the_z_axis():
    rs = np.random.RandomState(3)
    yaw = 0.5
    box = rs.uniform(-0.5, 0.5, (4000, 3)) * [4.5, 2.0, 1.6]
    turn = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    pts = (box @ turn.T + [30.0, -12.0, 0.8]).astype(np.float32)
    _, desc = D.describe(pts, np.zeros(len(pts), dtype=np.int32), 1, 1)
    a0, a1, a2 = desc[0, 6:9], desc[0, 9:12], desc[0, 12:15]
    assert a2.tolist() == [0.0, 0.0, 1.0] and a0[2] == 0.0 and a1.tolist() == [-a0[1], a0[0], 0.0]
    assert abs(np.arctan2(a0[1], a0[0]) - yaw) < 0.02
    extent = desc[0, 18:21] - desc[0, 15:18]
    assert np.abs(extent - [4.5, 2.0, 1.6]).max() < 0.05  # the axis-aligned box of the same car is 4.9 x 3.9
    assert np.abs(desc[0, 21:24] - [30.0, -12.0, 0.8]).max() < 0.05
    assert desc[0, 5] == pytest.approx(np.var(pts[:, 2].astype(np.float64)), rel=1e-4)  # lambda_2 = A_zz


def test_off_diagonals_are_exactly_zero_after_eight_sweeps():
    """covariances as the library forms them (integer moments of random lattice points, every shape from a line to a ball):
    after the eight sweeps the three off-diagonal entries are exactly 0.0, so the sorted diagonal IS the spectrum the model has"""
    rs = np.random.RandomState(0)
    for trial in range(2000):
        m = int(rs.randint(2, 40))
        spread = 2.0 ** rs.uniform(0, 20, 3)
        q = np.rint(np.abs(rs.standard_normal((m, 3)) * spread) @ np.abs(_rotation(rs).T)).astype(np.int64)
        _, A = D.covariance(D.moments_of(q), m)
        _, _, _, _, after = D.axes_of(A, 0)
        assert after[0, 1] == 0.0 and after[0, 2] == 0.0 and after[1, 2] == 0.0, (trial, after)
        _, _, _, _, after = D.axes_of(A, 1)
        assert after[0, 1] == 0.0


def test_moments_stay_below_two_to_the_62():
    for bitlen in range(1, 32):
        for m in {1 << (bitlen - 1), (1 << bitlen) - 1}:
            Q = D.lattice_bits(m)
            assert 15 <= Q <= 20 and m * (1 << Q) ** 2 < 2 ** 62, m
    m = 2 ** 22  # every member at the far corner of the lattice
    Q = D.lattice_bits(m)
    assert Q == 19
    S = D.moments_of(np.full((1, 3), 1 << Q, dtype=np.int64))
    assert all(v * m < 2 ** 62 for v in S) and S[3] * m == 2 ** 60


def test_model_edge_order_and_degenerate_cases():
    assert D.edge_corners() == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
    # E == 0: x = Q, h = 1, identity axes, a box of zero size at the point
    pts = np.full((3, 3), 7.25, dtype=np.float32)
    moments, desc = D.describe(pts, np.zeros(3, dtype=np.int32), 2, 0)
    assert moments[0].tolist() == [3] + [0] * 9 + [20, 20] and moments[1].tolist() == [0] * 12 and np.isnan(desc[1]).all()
    assert desc[0].tolist() == [7.25] * 3 + [0.0] * 3 + [1, 0, 0, 0, 1, 0, 0, 0, 1] + [0.0] * 6 + [7.25] * 3
    # -0.0 sorts below +0.0
    assert D.key_min(np.array([0.0, -0.0])).tobytes() == np.float64(-0.0).tobytes()
    assert D.key_max(np.array([-0.0, 0.0])).tobytes() == np.float64(0.0).tobytes()
    # a non-finite point is no member; ids outside [0, nclusters) are ignored
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [5, 5, 5], [9, 9, 9]], dtype=np.float32)
    moments, desc = D.describe(pts, np.array([0, 0, 0, -1, 1], dtype=np.int32), 1, 0)
    assert moments[0, 0] == 2 and desc[0, 0:3].tolist() == [0.5, 0.0, 0.0]
    w, owner = D.wireframe(desc, 3)
    assert w.shape == (36, 3) and owner.tolist() == [0] * 36 and w.dtype == np.float32
    assert w[0].tolist() == [0.0, 0.0, 0.0] and w[1].tolist() == [0.5, 0.0, 0.0] and w[2].tolist() == [1.0, 0.0, 0.0]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS and name not in pn2._lib._STATEFUL
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_cluster_describe_workspace_size"].argtypes == [i, p]
    assert fns["pn2_cluster_describe"].argtypes == [i, i, p, p, i, p, p, p, z, p]
    assert fns["pn2_box_wireframe"].argtypes == [i, p, i, p, p, p]
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_describe.hip" in pn2._lib._build.SOURCES
    with open(os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc", "pn2_describe.hip")) as src:
        assert "pn2_grid_knn.h" not in src.read()
    assert pn2.describe_clusters is pn2.cluster.describe_clusters and pn2.box_wireframe is pn2.cluster.box_wireframe
    assert pn2.Boxes is pn2.cluster.Boxes and pn2.Boxes._fields == ("size", "centroid", "variance", "axes", "center", "extent", "lo",
                                                                    "hi", "moments")


def _workspace_bytes(pn2, nclusters):
    nbytes = ctypes.c_ulonglong(0)
    assert pn2._lib.lib.pn2_cluster_describe_workspace_size(nclusters, ctypes.byref(nbytes)) == 0
    return int(nbytes.value)


def test_workspace_size(pn2):
    K = pn2._lib.ABI.constants
    query = pn2._lib.lib.pn2_cluster_describe_workspace_size
    nbytes = ctypes.c_ulonglong(7)
    assert query(0, ctypes.byref(nbytes)) == K["PN2_EINVAL"] and query(-4, ctypes.byref(nbytes)) == K["PN2_EINVAL"]
    assert query(100, None) == K["PN2_ENULL"] and nbytes.value == 7
    size = lambda c: _workspace_bytes(pn2, c)  # noqa: E731
    # per cluster: nine int64 sums, six box keys and a count (an atomics-only row), origin and lattice step, six extent keys
    assert size(1) % 256 == 0 and size(1) >= 3 * 256 and 9 * 8 + 7 * 4 + 4 * 8 + 6 * 8 <= size(1000) / 1000 <= 256
    assert size(1000) <= size(1001)


def _caller(pn2, name, good):
    names = pn2._lib.ABI.functions[name].argnames

    def call(**change):
        a = dict(good, **change)
        return getattr(pn2._lib.lib, name)(*[a[k] for k in names])
    return call


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL, ERANGE = K["PN2_EINVAL"], K["PN2_ENULL"], K["PN2_ERANGE"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    n, nclusters = 1000, 10
    need = _workspace_bytes(pn2, nclusters)
    # the good call would reach the stream query: every call below differs from it in at least one refused argument
    de = _caller(pn2, "pn2_cluster_describe", dict(n=n, nclusters=nclusters, points=fake, ids=fake, upright=0, moments=fake,
                                                   desc=fake, workspace=fake, workspace_bytes=need, stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(nclusters=0), dict(nclusters=-1), dict(upright=2), dict(upright=-1)):
        assert de(**bad) == EINVAL, bad
    assert de(nclusters=n + 1) == ERANGE
    for required in ("points", "ids", "moments", "desc", "workspace"):
        assert de(**{required: None}) == ENULL, required
    for k in ("points", "ids"):
        assert de(**{k: odd(2)}) == EINVAL, k
    for k in ("moments", "desc"):
        assert de(**{k: odd(4)}) == EINVAL, k
    assert de(workspace=odd(128)) == EINVAL and de(workspace_bytes=need - 1) == EINVAL and de(workspace_bytes=0) == EINVAL
    # the order: sizes, range, NULL, alignment and workspace
    assert de(upright=2, nclusters=n + 1) == EINVAL and de(nclusters=n + 1, ids=None) == ERANGE
    assert de(ids=None, workspace_bytes=0) == ENULL and de(desc=None, moments=odd(4)) == ENULL

    wf = _caller(pn2, "pn2_box_wireframe", dict(nclusters=nclusters, desc=fake, per_edge=8, points=fake, owner=fake, stream=None))
    for bad in (dict(nclusters=0), dict(nclusters=-3), dict(per_edge=1), dict(per_edge=0), dict(per_edge=-5)):
        assert wf(**bad) == EINVAL, bad
    assert wf(nclusters=1 << 20, per_edge=171) == ERANGE  # 2^20 * 12 * 171 >= 2^31 > 2^20 * 12 * 170
    assert wf(nclusters=(1 << 31) - 1, per_edge=(1 << 31) - 1) == ERANGE  # no overflow on the way to the answer
    for required in ("desc", "points", "owner"):
        assert wf(**{required: None}) == ENULL, required
    assert wf(desc=odd(4)) == EINVAL and wf(points=odd(2)) == EINVAL and wf(owner=odd(1)) == EINVAL
    assert wf(per_edge=1, desc=None) == EINVAL and wf(nclusters=1 << 20, per_edge=171, desc=None) == ERANGE
    assert wf(desc=None, points=odd(2)) == ENULL


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def _library_must_not_be_reached(pn2, monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pn2.cluster, "launch", fail)
    monkeypatch.setattr(pn2.cluster, "_on_device", fail)


def test_wrapper_argument_errors(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)  # (torch's own asks for a device)
    pts = np.zeros((10, 3), dtype=np.float32)
    ids = np.zeros((10,), dtype=np.int32)
    dc = pn2.describe_clusters
    for bad in (np.zeros((10, 4), dtype=np.float32), np.zeros((10,), dtype=np.float32), np.zeros((2, 5, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="points"):
            dc(bad, (ids, 1))
    for clusters, what in ((None, "clusters"), (ids, "clusters"), ((ids, 1, 2), "clusters"), ((ids, 1.0), "count"),
                           ((ids, True), "count"), ((ids, -1), "count"), ((ids, 11), "count"), ((ids[:9], 1), "ids"),
                           ((None, 1), "ids"), ((ids.astype(np.float32), 1), "ids: integers"),
                           ((torch.zeros(10, dtype=torch.bool), 1), "ids: integers"), (([0] * 10, 1), "ids")):
        with pytest.raises(ValueError, match=what):
            dc(pts, clusters)
    empty = pn2.cluster._empty_boxes(torch.device("cpu"))  # (a host stand-in: nothing is launched for no boxes)
    assert [tuple(t.shape) for t in empty] == [(0,), (0, 3), (0, 3), (0, 3, 3), (0, 3), (0, 3), (0, 3), (0, 3), (0, 12)]
    assert empty.size.dtype == torch.int64 and empty.moments.dtype == torch.int64 and empty.axes.dtype == torch.float64
    assert empty.corners().shape == (0, 8, 3) and empty.yaw().shape == (0,)
    for per_edge in (1, 0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="per_edge"):
            pn2.box_wireframe(empty, per_edge)
    with pytest.raises(ValueError, match="boxes"):
        pn2.box_wireframe((1, 2, 3))
    points, owner = pn2.box_wireframe(empty, 4)  # no boxes: empty tensors, no launch
    assert points.shape == (0, 3) and owner.shape == (0,) and points.dtype == torch.float32 and owner.dtype == torch.int32


def test_wrapper_refuses_a_capturing_stream(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.describe_clusters(np.zeros((10, 3), dtype=np.float32), (np.zeros(10, dtype=np.int32), 1))
    with pytest.raises(RuntimeError, match="capturing"):  # before the arguments are looked at
        pn2.describe_clusters(np.zeros((10, 4), dtype=np.float32), None)


def test_boxes_helpers_on_host_tensors(pn2):
    """corners() and yaw() are plain torch ops over the namedtuple's fields: checked against the model's corners on the host"""
    import torch
    rs = np.random.RandomState(1)
    pts = np.concatenate([_cloud(rs, 50, np.array([5.0, -3.0, 1.0])), _cloud(rs, 70, np.zeros(3))])
    ids = np.repeat([0, 1], [50, 70]).astype(np.int32)
    moments, desc = D.describe(pts, ids, 2, 0)
    boxes = pn2.cluster._boxes_of(torch.from_numpy(moments), torch.from_numpy(desc))
    assert boxes.size.tolist() == [50, 70] and boxes.axes.shape == (2, 3, 3)
    assert torch.equal(boxes.extent, boxes.hi - boxes.lo) and torch.equal(boxes.center, torch.from_numpy(desc[:, 21:24]))
    want = np.array([[D.corner(desc[c], j) for j in range(8)] for c in range(2)])
    assert np.abs(boxes.corners().numpy() - want).max() < 1e-12 * np.abs(want).max()
    assert np.allclose(boxes.yaw().numpy(), np.arctan2(desc[:, 7], desc[:, 6]))
