"""CPU tests of rigid registration (csrc/pn2_icp.hip, icp.py): the numpy model of the rules (tests/icp_ref.py) against independent
code -- numpy's SVD Kabsch for one Horn step, np.linalg.solve for one point-to-plane step, a known motion for the whole loop --,
the header's prototypes, pn2_icp_workspace_size's refusals and monotonicity, every refusal of pn2_icp and pn2_transform_points
that needs no GPU and their order, the wrappers' argument errors and their refusal of a capturing stream.  Nothing here needs a
GPU.

The tolerances of the model-only checks are not fixed numbers: each test measures how far the independent numpy answer itself
lies from the truth on its data (the float32 rounding of the clouds, the linearisation) and allows the model 8x that, because
the Jacobi and Cholesky results differ from numpy's only by rounding.  The measured values are in the tests' docstrings."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_ref as R  # noqa: E402
from icp_cases import TRUTH, corner, corner_bound, kabsch, moved_corner, rigid  # noqa: E402

F = np.float64
ARGS = {
    "pn2_icp_workspace_size": ("ns", "nt", "max_iteration", "bytes"),
    "pn2_icp": ("ns", "source", "source_labels", "nt", "target", "target_labels", "target_normals", "max_distance", "estimation",
                "init", "max_iteration", "relative_fitness", "relative_rmse", "correspondence", "result", "trace", "header",
                "workspace", "workspace_bytes", "stream"),
    "pn2_transform_points": ("n", "points", "transform", "out", "stream"),
}


# ---- the model against independent code ----------------------------------------------------------------------------------------
def test_one_horn_step_against_svd_kabsch():
    """exact pairs (index i with i), 300 points, a 25 degree rotation: numpy's SVD answer lies 2.65e-08 (max entry of the 4x4)
    from the truth -- the float32 rounding of both clouds --, the model's Horn step 2.65e-08, and the two 6.1e-15 from each
    other; the bound is 8 x 2.65e-08"""
    rs = np.random.RandomState(1)
    truth = rigid([0.3, -1.0, 0.5], 25.0, [0.4, -0.2, 0.1])
    p = (rs.uniform(-1, 1, (300, 3)) * [2.0, 1.0, 0.5] + [5.0, 5.0, -3.0]).astype(np.float32)
    u = (p.astype(F) @ truth[:3, :3].T + truth[:3, 3]).astype(np.float32)
    want = kabsch(p.astype(F), u.astype(F))
    dev = np.abs(want - truth).max()
    o = u.astype(F).min(0)
    index = np.arange(300, dtype=np.int32)
    d = u.astype(F) - p.astype(F)
    S = R.tree_sum(R.lane_rows(0, p, index, (d * d).sum(1), u.astype(F), None, o))
    assert S[0] == 300
    Rm, t = R.solve_point(S, o)
    got = R.compose(Rm, t, np.eye(4))
    print("svd-truth %.3g model-truth %.3g model-svd %.3g" % (dev, np.abs(got - truth).max(), np.abs(got - want).max()))
    assert 0 < dev < 1e-6 and np.abs(got - truth).max() <= 8 * dev
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14
    # the sweeps end exactly diagonal on this matrix, and the quaternion belongs to the largest eigenvalue
    N = np.random.RandomState(2).standard_normal((4, 4))
    N = N + N.T
    q, after = R.largest_eigenvector(N)
    assert np.abs(after - np.diag(np.diag(after))).max() == 0.0
    lam = np.linalg.eigvalsh(N)
    assert abs(after.diagonal().max() - lam[-1]) < 1e-14 and np.abs(N @ q - lam[-1] * q).max() < 1e-14


def test_one_plane_step_against_linalg_solve():
    """the corner under a 0.1 degree, 0.002 unit motion, exact pairs: np.linalg.solve's (a, b, c, tx, ty, tz) lies 8.09e-07 from
    the true small motion (the linearisation and the float32 rounding), the model's Cholesky 8.09e-07, the two 6.5e-19 from each
    other; the bound is 8 x 8.09e-07"""
    target, normals = corner(3)
    small = rigid([2, -1, 1], 0.1, [0.001, -0.0015, 0.001])
    inv = np.linalg.inv(small)
    source = (target.astype(F) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    o = target.astype(F).min(0)
    index = np.arange(len(source), dtype=np.int32)
    d = target.astype(F) - source.astype(F)
    S = R.tree_sum(R.lane_rows(1, source, index, (d * d).sum(1), target.astype(F), normals, o))
    A, g = R.plane_system(S)
    want = np.linalg.solve(A, -g)
    got = R.cholesky_solve(A, g)
    # the true motion in the model's parametrisation: rotation vector (to first order) and the translation of the points about o
    Rt = small[:3, :3]
    true = np.concatenate([[Rt[2, 1] - Rt[1, 2], Rt[0, 2] - Rt[2, 0], Rt[1, 0] - Rt[0, 1]], small[:3, 3] - o + Rt @ o])
    true[:3] /= 2.0
    dev = np.abs(want - true).max()
    print("solve-truth %.3g model-truth %.3g model-solve %.3g" % (dev, np.abs(got - true).max(), np.abs(got - want).max()))
    assert 0 < dev < 1e-5 and np.abs(got - true).max() <= 8 * dev
    Rm, t = R.solve_plane(S, o)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14
    # a pivot that is not positive: all normals parallel leaves the in-plane motion free
    flat = normals.copy()
    flat[:] = [0, 0, 1]
    S = R.tree_sum(R.lane_rows(1, source, index, (d * d).sum(1), target.astype(F), flat, o))
    assert R.solve_plane(S, o) is None


@pytest.mark.parametrize("estimation", [0, 1])
def test_model_converges_to_a_known_motion(estimation):
    """moved_corner(): numpy's Kabsch on the true pairs lies 1.75e-08 from TRUTH, so the bound is 1.4e-07; the model's final
    pose lies 1.77e-08 (point-to-point, 5 updates) and 2.66e-08 (point-to-plane, 4 updates) from it"""
    source, target, normals = moved_corner()
    bound = corner_bound()
    out = R.icp(source, target, 0.5, estimation, None, 30, 1e-6, 1e-6, target_normals=normals)
    err = np.abs(out.result[:16].reshape(4, 4) - TRUTH).max()
    print("bound %.3g error %.3g header %s" % (bound, err, out.header.tolist()))
    assert out.header[0] == 0 and out.header[5] == 1 and 1 <= out.header[4] < 30 and out.header[3] == 400
    assert 0 < bound < 1e-6 and err <= bound
    assert out.correspondence.tolist() == list(range(400)) and out.result[16] == 1.0
    k = out.header[4]
    assert (out.trace[k + 1:] == 0).all() and (out.trace[:k + 1, 0] > 0).all() and out.trace[k, 2] == out.result[17]
    assert out.trace[0, 2] > 0.05 and out.result[17] < 1e-6  # from a tenth of a unit to float32 noise


def test_model_hand_made_cases():
    tgt = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9]], dtype=np.float32)
    src = np.array([[0.1, 0, 0], [0.5, 0, 0], [4, 4, 4], [np.nan, 0, 0], [0, 0.9, 0]], dtype=np.float32)
    out = R.icp(src, tgt, 0.5, max_iteration=0)
    # the tie at (0.5, 0, 0) goes to the lower index; (4,4,4) has no partner; the NaN row is invalid
    assert out.correspondence.tolist() == [0, 0, -1, -1, 2] and out.header.tolist() == [0, 4, 5, 3, 0, 0, 0, 0]
    assert out.result[16] == 0.75 and out.result[18] == F(np.float32(0.1)) ** 2 + 0.25 + (F(np.float32(0.9)) - 1) ** 2
    assert np.array_equal(out.result[:16].reshape(4, 4), np.eye(4)) and out.trace.shape == (1, 20)
    # status 2: two pairs do not make a rotation
    out = R.icp(src[:2], tgt, 0.5, max_iteration=5)
    assert out.header.tolist() == [2, 2, 5, 2, 0, 0, 0, 0] and np.array_equal(out.result[:16].reshape(4, 4), np.eye(4))
    # status 1: the target does not fit the grid
    wide = np.array([[0, 0, 0], [1e7, 0, 0]], dtype=np.float32)
    init = rigid([0, 0, 1], 30.0, [1, 2, 3])
    out = R.icp(src, wide, 1.0, init=init, max_iteration=3)
    assert out.header.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (out.correspondence == -1).all()
    assert np.array_equal(out.result[:16].reshape(4, 4), init) and (out.result[16:] == 0).all()
    assert (out.trace[0, :4] == 0).all() and np.array_equal(out.trace[0, 4:].reshape(4, 4), init) and (out.trace[1:] == 0).all()
    # the transform: float64, rounded once; invalid rows pass through
    moved = R.transform_points(src, init)
    assert np.isnan(moved[3, 0]) and moved[3, 1:].tolist() == [0, 0]
    want = (src[[0, 1, 2, 4]].astype(F) @ init[:3, :3].T + init[:3, 3])
    assert np.abs(moved[[0, 1, 2, 4]] - want).max() < 1e-6


def test_the_tree_is_the_headers():
    """the sum of 2^52, 1 and -2^52 in the order of the tree, not in index order: lanes 0, 1, 32 of wave 0"""
    rows = np.zeros((300, 1))
    rows[0], rows[1], rows[32] = 2.0 ** 53, 1.0, -2.0 ** 53
    # xor 32 pairs lane 0 with lane 32 first: (2^53 - 2^53) + 1 = 1; in index order the 1 would be lost
    assert R.tree_sum(rows)[0] == 1.0 and (rows[0] + rows[1]) + rows[32] == 0.0
    rows = np.zeros((600, 1))
    rows[0], rows[64], rows[256] = 2.0 ** 53, 1.0, -2.0 ** 53
    assert R.tree_sum(rows)[0] == 0.0  # (w0 + w1) rounds the 1 away before workgroup 1 arrives


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS and name not in pn2._lib._STATEFUL
    i, f, d, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_icp_workspace_size"].argtypes == [i, i, i, p]
    assert fns["pn2_icp"].argtypes == [i, p, p, i, p, p, p, f, i, p, i, d, d, p, p, p, p, p, z, p]
    assert fns["pn2_transform_points"].argtypes == [i, p, p, p, p]
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_icp.hip" in pn2._lib._build.SOURCES
    csrc = os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc")
    for name in ("pn2_icp.hip", "pn2_eig4.h"):
        with open(os.path.join(csrc, name)) as src:
            text = src.read()
        assert "pn2_grid_knn.h" not in text and "hipMalloc" not in text and "hipMemset" not in text, name
    for name in ("registration_icp", "evaluate_registration", "transform_points", "RegistrationResult"):
        assert getattr(pn2, name) is getattr(pn2.icp, name), name
    assert pn2.RegistrationResult._fields == ("transformation", "fitness", "inlier_rmse", "correspondence", "iterations", "converged",
                                              "status", "trace")
    assert callable(pn2.kitti_predict.PredictInterpolator.align_frames)


def _workspace_bytes(pn2, ns, nt, max_iteration=30):
    nbytes = ctypes.c_ulonglong(0)
    assert pn2._lib.lib.pn2_icp_workspace_size(ns, nt, max_iteration, ctypes.byref(nbytes)) == 0
    return int(nbytes.value)


def test_workspace_size(pn2):
    K = pn2._lib.ABI.constants
    query = pn2._lib.lib.pn2_icp_workspace_size
    nbytes = ctypes.c_ulonglong(7)
    for bad in ((0, 10, 1), (10, 0, 1), (-1, 10, 1), (10, -5, 1), (10, 10, -1)):
        assert query(*bad, ctypes.byref(nbytes)) == K["PN2_EINVAL"], bad
    assert query(100, 100, 3, None) == K["PN2_ENULL"] and query(0, 100, 3, None) == K["PN2_EINVAL"] and nbytes.value == 7
    size = lambda ns, nt, it=30: _workspace_bytes(pn2, ns, nt, it)  # noqa: E731
    # per target point: two keys, two indices, one label and one (x, y, z, index) row; per 256 source points a row of 32 doubles
    assert size(1, 1) % 256 == 0 and size(1, 1000) >= 1000 * (2 * 8 + 3 * 4 + 16) and size(5000, 1) >= 20 * 32 * 8
    for ns, nt in ((1, 1), (255, 64), (256, 65), (1000, 1000), (50000, 1000)):
        base = size(ns, nt)
        assert size(ns + 1, nt) >= base and size(ns, nt + 1) >= base and size(ns + 257, nt) > base
        assert size(ns, nt, 0) <= base <= size(ns, nt, 31)


def _good(pn2, fake, need, n=1000):
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    return dict(ns=n, source=fake, source_labels=fake, nt=n, target=fake, target_labels=fake, target_normals=fake, max_distance=0.5,
                estimation=1, init=eye, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, correspondence=fake,
                result=fake, trace=fake, header=fake, workspace=fake, workspace_bytes=need, stream=None)


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL = K["PN2_EINVAL"], K["PN2_ENULL"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    n = 1000
    need = _workspace_bytes(pn2, n, n)
    names = pn2._lib.ABI.functions["pn2_icp"].argnames
    good = _good(pn2, fake, need)

    def matrix(at, value):  # (init is host memory and IS read)
        m = np.eye(4).reshape(-1)
        m[at] = value
        return (ctypes.c_double * 16)(*m)

    def call(**change):
        a = dict(good, **change)
        return pn2._lib.lib.pn2_icp(*[a[k] for k in names])

    nan, inf = float("nan"), float("inf")
    for bad in (dict(ns=0), dict(ns=-1), dict(nt=0), dict(nt=-7), dict(max_distance=0.0), dict(max_distance=-1.0),
                dict(max_distance=inf), dict(max_distance=nan), dict(estimation=2), dict(estimation=-1), dict(max_iteration=-1),
                dict(relative_fitness=nan), dict(relative_fitness=-1e-9), dict(relative_rmse=nan), dict(relative_rmse=-1.0),
                dict(init=matrix(0, nan)), dict(init=matrix(7, inf)), dict(init=matrix(15, -inf))):
        assert call(**bad) == EINVAL, bad
    for required in ("source", "target", "target_normals", "correspondence", "result", "header", "workspace"):
        assert call(**{required: None}) == ENULL, required
    for k in ("source", "source_labels", "target", "target_labels", "target_normals", "correspondence", "header"):
        assert call(**{k: odd(2)}) == EINVAL, k
    for k in ("result", "trace"):
        assert call(**{k: odd(4)}) == EINVAL, k
    assert call(workspace=odd(128)) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    # optional arguments may be NULL: what remains wrong is still what is reported; point-to-point needs no normals
    free = dict(source_labels=None, target_labels=None, init=None, trace=None)
    assert call(workspace_bytes=0, **free) == EINVAL and call(header=None, **free) == ENULL
    assert call(estimation=0, target_normals=None, workspace_bytes=0, **free) == EINVAL
    assert call(estimation=0, target_normals=odd(2)) == EINVAL
    # the order: values (init among them), NULL, alignment and workspace
    assert call(max_distance=0.0, source=None) == EINVAL and call(init=matrix(3, nan), result=None) == EINVAL
    assert call(max_iteration=-1, workspace=odd(128)) == EINVAL
    assert call(header=None, workspace_bytes=0) == ENULL and call(target_normals=None, trace=odd(4)) == ENULL
    assert call(correspondence=None, source=odd(2)) == ENULL

    tp = pn2._lib.lib.pn2_transform_points
    eye = good["init"]
    assert tp(0, fake, eye, fake, None) == EINVAL and tp(-3, fake, eye, fake, None) == EINVAL
    assert tp(10, None, eye, fake, None) == ENULL and tp(10, fake, None, fake, None) == ENULL and tp(10, fake, eye, None, None) == ENULL
    assert tp(10, fake, matrix(5, nan), fake, None) == EINVAL and tp(10, fake, matrix(12, inf), fake, None) == EINVAL
    assert tp(10, odd(2), eye, fake, None) == EINVAL and tp(10, fake, eye, odd(1), None) == EINVAL
    assert tp(0, None, eye, fake, None) == EINVAL and tp(10, None, matrix(5, nan), fake, None) == ENULL


# ---- the wrappers --------------------------------------------------------------------------------------------------------------
def _library_must_not_be_reached(pn2, monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pn2.icp, "launch", fail)
    monkeypatch.setattr(pn2.neighbors, "launch", fail)
    monkeypatch.setattr(pn2.cluster, "_on_device", fail)
    monkeypatch.setattr(pn2.cluster, "_device_of", fail)


def test_wrapper_argument_errors(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)  # (torch's own asks for a device)
    pts = np.zeros((10, 3), dtype=np.float32)
    icp = pn2.registration_icp
    for bad in (np.zeros((10, 4), dtype=np.float32), np.zeros((10,), dtype=np.float32)):
        with pytest.raises(ValueError, match="points"):
            icp(bad, pts, 0.5)
        with pytest.raises(ValueError, match="points"):
            icp(pts, bad, 0.5)
        with pytest.raises(ValueError, match="points"):
            pn2.transform_points(bad, np.eye(4))
    for d in (0.0, -1.0, float("nan"), float("inf"), 1e39, "wide", None):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            icp(pts, pts, d)
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            pn2.evaluate_registration(pts, pts, d)
    with pytest.raises(ValueError, match="estimation"):
        icp(pts, pts, 0.5, estimation="plane")
    for m in (-1, 2.0, True, None, 2 ** 20):
        with pytest.raises(ValueError, match="max_iteration"):
            icp(pts, pts, 0.5, max_iteration=m)
    for name in ("relative_fitness", "relative_rmse"):
        for v in (-1e-9, float("nan"), "small"):
            with pytest.raises(ValueError, match=name):
                icp(pts, pts, 0.5, **{name: v})
    for T in (np.eye(3), np.full((4, 4), np.nan), [1, 2, 3], "identity"):
        with pytest.raises(ValueError, match="init"):
            icp(pts, pts, 0.5, init=T)
        with pytest.raises(ValueError, match="transformation"):
            pn2.transform_points(pts, T)
    with pytest.raises(ValueError, match="transformation"):
        pn2.transform_points(pts, None)
    with pytest.raises(ValueError, match="target_normals"):
        icp(pts, pts, 0.5, estimation="point_to_plane")
    with pytest.raises(ValueError, match="target_normals"):
        icp(pts, pts, 0.5, estimation="point_to_plane", target_normals=np.zeros((9, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="labels"):
        icp(pts, pts, 0.5, source_labels=np.zeros(9, dtype=np.int32))
    with pytest.raises(ValueError, match="labels: integers"):
        icp(pts, pts, 0.5, target_labels=np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError, match="classes"):
        icp(pts, pts, 0.5, classes=[1])
    with pytest.raises(ValueError, match="classes"):
        icp(pts, pts, 0.5, source_labels=np.zeros(10, dtype=np.int32), classes=[1])
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)
    frame = type("Frame", (), {"points": pts})()
    with pytest.raises(ValueError, match="classes"):
        predictor.align_frames(frame, frame, 0.5, classes=[1], dense_labels=np.zeros(10, dtype=np.int32))


def test_wrappers_refuse_a_capturing_stream(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    pts = np.zeros((10, 3), dtype=np.float32)
    for call in (lambda p, d: pn2.registration_icp(p, p, d), lambda p, d: pn2.evaluate_registration(p, p, d)):
        with pytest.raises(RuntimeError, match="capturing"):
            call(pts, 0.5)
        with pytest.raises(RuntimeError, match="capturing"):  # before the arguments are looked at
            call(np.zeros((10, 4), dtype=np.float32), -1.0)
    frame = type("Frame", (), {"points": pts})()
    predictor = object.__new__(pn2.kitti_predict.PredictInterpolator)
    with pytest.raises(RuntimeError, match="capturing"):
        predictor.align_frames(frame, frame, 0.5)
    with pytest.raises(RuntimeError, match="capturing"):
        predictor.align_frames(frame, frame, 0.5, estimation="point_to_plane")


def test_pose_helpers_on_the_host(pn2):
    A, B = rigid([0, 0, 1], 90.0, [1, 0, 0]), rigid([1, 0, 0], 10.0, [0, 2, 0])
    assert np.allclose(pn2.icp.compose(A, B), A @ B) and np.array_equal(pn2.icp.compose(), np.eye(4))
    angle, dist = pn2.icp.rigid_error(A, np.eye(4))
    assert abs(angle - 90.0) < 1e-9 and abs(dist - 1.0) < 1e-12
    assert pn2.icp.rigid_error(B, B) == (0.0, 0.0) or max(pn2.icp.rigid_error(B, B)) < 1e-7
