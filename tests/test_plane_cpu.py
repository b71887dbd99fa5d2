"""CPU tests of plane segmentation (csrc/pn2_plane.hip, plane.py): the numpy model of the rules (tests/plane_ref.py) against brute
force in Python floats on tiny clouds and against hand-made cases, the header's prototypes and the binding, the refusals of the
entry points with placeholder pointers, the wrapper's argument errors, the capturing-stream refusal as the header states it, and
the index table of csrc/pn2_rng.h.  Nothing here needs a GPU."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_ref as R  # noqa: E402
from dataset_stream_ref import draw64, sample_stream  # noqa: E402

CSRC = os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc")
ARGS = {
    "pn2_plane_score": ("n", "points", "labels", "nplanes", "planes", "thr", "counts", "stream"),
    "pn2_plane_workspace_size": ("n", "trials", "bytes"),
    "pn2_plane_ransac": ("n", "points", "labels", "thr", "trials", "seed", "axis", "cos2", "inlier", "plane", "header", "workspace",
                         "workspace_bytes", "stream"),
}


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _brute_ransac(points, thr, trials, seed, labels=None, axis=None, cos2=0.0):
    """the rules once more, point by point in Python floats (IEEE doubles, one rounding per operation) and Python integers"""
    n = len(points)
    P = [[float(v) for v in row] for row in points]
    ok = [all(math.isfinite(v) for v in P[i]) and (labels is None or labels[i] >= 0) for i in range(n)]
    valid = [i for i in range(n) if ok[i]]
    V = len(valid)
    if V < 3:
        return [0] * n, None, [1, 0, 0, -1, -1, -1, V, 0]
    h = int(sample_stream(seed, 0, 0)[0])
    thr2 = float(np.float32(thr)) * float(np.float32(thr))
    best, live = None, 0
    for t in range(trials):
        s = [valid[int(draw64(h, 2 ** 45 + 3 * t + j)[0]) % V] for j in range(3)]
        A, B, C = P[s[0]], P[s[1]], P[s[2]]
        u, v = [B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]
        a, b, c = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
        nn = (a * a + b * b) + c * c
        if not (math.isfinite(nn) and nn > 0):
            continue
        if axis is not None:
            dt = (a * axis[0] + b * axis[1]) + c * axis[2]
            if not dt * dt >= (cos2 * nn) * ((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]):
                continue
        live += 1
        mask = []
        for i in range(n):
            e = (a * (P[i][0] - A[0]) + b * (P[i][1] - A[1])) + c * (P[i][2] - A[2]) if ok[i] else float("nan")
            mask.append(1 if e * e <= thr2 * nn else 0)
        if best is None or sum(mask) > best[0]:
            best = (sum(mask), t, s, mask, (a, b, c, -((a * A[0] + b * A[1]) + c * A[2])))
    if best is None:
        return [0] * n, None, [2, 0, 0, -1, -1, -1, V, 0]
    count, t, s, mask, (a, b, c, d) = best
    flip = ((a * axis[0] + b * axis[1]) + c * axis[2] < 0) if axis is not None else (c < 0 if c != 0 else (b < 0 if b != 0 else a < 0))
    plane = [-a, -b, -c, -d] if flip else [a, b, c, d]
    return mask, plane, [0, count, t] + s + [V, live]


@pytest.mark.parametrize("n,trials,seed,with_labels,axis", [(3, 1, 0, False, None), (4, 5, 1, False, None), (40, 30, 2, True, None),
                                                            (65, 17, 3, True, (0.0, 0.0, 1.0)), (30, 64, 4, False, (1.0, 2.0, -0.5))])
def test_model_against_brute_force(n, trials, seed, with_labels, axis):
    rs = np.random.RandomState(100 + n)
    pts = (rs.random_sample((n, 3)) * [4.0, 4.0, 0.3]).astype(np.float32)
    labels = rs.randint(-1, 3, n).astype(np.int32) if with_labels else None
    if n > 10:
        pts[n // 3, 1], pts[n // 2, 0] = np.nan, np.inf
    cos2 = R.cos2_of(40.0)
    mask, plane, header = R.ransac(pts, 0.05, trials, seed, labels, axis, cos2)
    want_mask, want_plane, want_header = _brute_ransac(pts, 0.05, trials, seed, labels, axis, cos2)
    assert header.tolist() == want_header and mask.tolist() == want_mask
    if want_plane is None:
        assert plane.tolist() == [0.0] * 4
    else:
        assert plane.tobytes() == np.array(want_plane, dtype=np.float64).tobytes()
        assert header[1] == mask.sum() >= 1 and mask[header[3]] == 1


def test_model_on_hand_made_cases():
    # the plane z = 0 through integer points, thr = 0.5: 0.5 is inside, one ulp above it is outside; invalid points never count
    above = np.nextafter(np.float32(0.5), np.float32(1))
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 4, 0.5], [3, 4, above], [5, 5, -0.5], [np.nan, 0, 0], [0, np.inf, 0]],
                   dtype=np.float32)
    for scale in (1.0, 3.0, 1e-3, 1e150):  # the normal need not be of unit length
        plane = np.array([7.0, -2.0, 0.0, 0.0, 0.0, scale])
        assert R.inliers(pts, plane, 0.5).tolist() == [True, True, True, True, False, True, False, False]
        assert R.score(pts, plane[None], 0.5).tolist() == [5]
    assert R.score(pts, np.array([[0, 0, 0, 0, 0, 1.0]]), 0.5, np.array([0, -1, 2, -5, 0, 0, 0, 0])).tolist() == [3]
    # void planes: a zero normal, NaN and inf in it, nn overflowing
    void = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, np.nan, 0, 1], [0, 0, 0, 0, np.inf, 0], [0, 0, 0, 1e200, 0, 1]], dtype=np.float64)
    assert R.score(pts, void, 0.5).tolist() == [0, 0, 0, 0]
    # 1e30 next to ordinary coordinates: large, finite, far from the plane
    far = np.array([[0, 0, 0], [1e30, 0, 0], [0, 1e30, 0.25], [1e30, 1e30, 1e30]], dtype=np.float32)
    assert R.inliers(far, np.array([0, 0, 0, 0, 0, 1.0]), 0.5).tolist() == [True, True, True, False]
    # orientation: with an axis dt >= 0, without one the first non-zero of (c,b,a) is positive
    assert R.orient([1, 2, 3, 0, 0, -2.0]).tolist() == [0, 0, 2, -6]
    assert R.orient([1, 2, 3, 0, -1.0, 0]).tolist() == [0, 1, 0, -2]
    assert R.orient([1, 2, 3, -4.0, 0, 0]).tolist() == [4, 0, 0, -4]
    assert R.orient([1, 2, 3, -4.0, 5.0, 0]).tolist() == [-4, 5, 0, -6]
    assert R.orient([1, 2, 3, 0, 0, 2.0], axis=(0, 0, -1)).tolist() == [0, 0, -2, 6]
    assert R.orient([1, 2, 3, 1.0, 0, 0], axis=(0, 0, 1)).tolist() == [1, 0, 0, -1]  # dt == 0 stays
    # statuses
    two = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0]], dtype=np.float32)
    mask, plane, header = R.ransac(two, 0.1, 8)
    assert header.tolist() == [1, 0, 0, -1, -1, -1, 2, 0] and not mask.any() and plane.tolist() == [0] * 4
    line = np.outer(np.arange(50), [1.0, 2.0, -0.5]).astype(np.float32)  # exact in float32: every cross product is zero
    mask, plane, header = R.ransac(line, 0.1, 40)
    assert header.tolist() == [2, 0, 0, -1, -1, -1, 50, 0] and not mask.any() and plane.tolist() == [0] * 4


def test_model_finds_a_planted_ground():
    """3000 points, 1800 of them a ground of slope 0.02 with noise 0.03, thr 0.05, 64 trials, seed 7.  The header is pinned from
    this model (the cloud of the issue's prototype, trial 15 with 1646 inliers, was not recorded): it guards the model and the
    device against drifting together; what is independent of the model are the assertions after it and the brute-force cases."""
    pts = R.planted()
    mask, plane, header = R.ransac(pts, 0.05, 64, 7)
    assert header.tolist() == [0, 1539, 14, 1377, 530, 619, 3000, 64]
    assert mask[:1800].sum() > 1500 and mask[1800:].sum() < 20  # the ground, not the clutter
    unit = plane / np.sqrt((plane[:3] ** 2).sum())
    assert unit[2] > 0.999 and abs(unit[0] + 0.02) < 0.01 and abs(unit[3]) < 0.05


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS and name not in pn2._lib._STATEFUL
    i, f, d, p, z, u = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_ulonglong
    assert fns["pn2_plane_score"].argtypes == [i, p, p, i, p, f, p, p]
    assert fns["pn2_plane_workspace_size"].argtypes == [i, i, p]
    assert fns["pn2_plane_ransac"].argtypes == [i, p, p, f, i, u, p, d, p, p, p, p, z, p]
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_plane.hip" in pn2._lib._build.SOURCES
    with open(os.path.join(CSRC, "pn2_plane.hip")) as src:
        text = src.read()
    assert "pn2_grid_knn.h" not in text and "hipcub" not in text and "hipMemset" not in text  # no search, no sort, no memset node
    assert "hipMalloc" not in text and "hipGraph" not in text
    for name in ("segment_plane", "segment_planes", "score_planes", "Plane"):
        assert getattr(pn2, name) is getattr(pn2.plane, name)
    assert set(pn2.plane.STATUS_NAMES) == {1, 2}


def test_capturing_stream_refusal_is_stated(pn2):
    """the refusal is read, not provoked: the header says both entry points refuse a capturing stream, the source asks the
    stream in both before its first launch, and DESIGN.md says the refusal is to be lifted by a later change"""
    with open(pn2.build.HEADER) as f:
        header = f.read()
    section = header[header.index("/* Plane segmentation"):]
    assert re.search(r"Both pn2_plane_score and pn2_plane_ransac refuse a capturing stream", section)
    assert section.count("PN2_EUNSUP") >= 2  # once in the refusals of each entry point
    with open(os.path.join(CSRC, "pn2_plane.hip")) as f:
        text = f.read()
    for entry in ("pn2_plane_score", "pn2_plane_ransac"):
        body = text[text.index('extern "C" int %s(' % entry):]
        body = body[:body.index("\n}\n")]
        assert body.index("refuse_capture(st)") < body.index("launch_score(")
        assert "<<<" not in body[:body.index("refuse_capture(st)")]
    with open(os.path.join(CSRC, "pn2_wg.h")) as f:  # refuse_capture lives with the other host helpers, in one copy
        helper = f.read()
    helper = helper[helper.index("inline int refuse_capture(hipStream_t st)"):]
    helper = helper[:helper.index("\n}\n")]
    assert "hipStreamIsCapturing(st" in helper and "PN2_EUNSUP" in helper and "int refuse_capture(" not in text
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert re.search(r"plane.*refuse[sd]? a capturing stream", f.read(), re.S | re.I)


def test_rng_index_table_names_the_range():
    with open(os.path.join(CSRC, "pn2_rng.h")) as f:
        head = f.read().split("#pragma once")[0]
    assert "[2^45, 2^46)" in head and "pn2_plane.hip" in head
    assert R.RANK_TAG == 2 ** 45
    # and no other user's range reaches it
    assert "[2^41, 2^45)" in head


def _workspace_bytes(pn2, n, trials):
    nbytes = ctypes.c_ulonglong(0)
    assert pn2._lib.lib.pn2_plane_workspace_size(n, trials, ctypes.byref(nbytes)) == 0
    return int(nbytes.value)


def test_workspace_size(pn2):
    K = pn2._lib.ABI.constants
    query = pn2._lib.lib.pn2_plane_workspace_size
    nbytes = ctypes.c_ulonglong(7)
    for n, trials in ((0, 10), (-4, 10), (10, 0), (10, -1), (10, 2 ** 20 + 1)):
        assert query(n, trials, ctypes.byref(nbytes)) == K["PN2_EINVAL"], (n, trials)
    assert query(100, 10, None) == K["PN2_ENULL"] and nbytes.value == 7
    size = lambda n, t: _workspace_bytes(pn2, n, t)  # noqa: E731
    # the scalars, a count per block of 256 points, an index per point, 6 doubles and a count per trial: each rounded up to 256
    assert size(1, 1) == 5 * 256
    assert 4 * 1000 + 52 * 64 <= size(1000, 64) <= 4 * 1000 + 52 * 64 + 6 * 256
    assert size(1000, 64) <= size(1001, 64) <= size(1001, 2 ** 20) and size(2 ** 31 - 1, 2 ** 20) > 2 ** 33


def _caller(pn2, name, good):
    names = pn2._lib.ABI.functions[name].argnames

    def call(**change):
        a = dict(good, **change)
        return getattr(pn2._lib.lib, name)(*[a[k] for k in names])
    return call


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL = K["PN2_EINVAL"], K["PN2_ENULL"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    n, trials = 1000, 64
    need = _workspace_bytes(pn2, n, trials)
    axis = lambda *v: (ctypes.c_double * 3)(*v)  # noqa: E731

    sc = _caller(pn2, "pn2_plane_score", dict(n=n, points=fake, labels=fake, nplanes=10, planes=fake, thr=0.5, counts=fake,
                                              stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(nplanes=0), dict(nplanes=-3), dict(nplanes=2 ** 24 + 1), dict(nplanes=2 ** 31 - 1),
                dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
                dict(thr=float("inf"))):
        assert sc(**bad) == EINVAL, bad
    for required in ("points", "planes", "counts"):
        assert sc(**{required: None}) == ENULL, required
    for k, by in (("points", 2), ("labels", 2), ("counts", 2), ("planes", 4)):
        assert sc(**{k: odd(by)}) == EINVAL, k
    assert sc(n=0, points=None) == EINVAL and sc(counts=None, planes=odd(4)) == ENULL

    rn = _caller(pn2, "pn2_plane_ransac", dict(n=n, points=fake, labels=fake, thr=0.5, trials=trials, seed=1, axis=None, cos2=0.0,
                                               inlier=fake, plane=fake, header=fake, workspace=fake, workspace_bytes=need,
                                               stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(trials=0), dict(trials=-1), dict(trials=2 ** 20 + 1), dict(thr=0.0), dict(thr=-0.5),
                dict(thr=float("nan")), dict(thr=float("inf")),
                dict(axis=axis(0, 0, 1), cos2=-0.1), dict(axis=axis(0, 0, 1), cos2=1.5), dict(axis=axis(0, 0, 1), cos2=float("nan")),
                dict(axis=axis(0, 0, 0), cos2=0.5), dict(axis=axis(0, float("nan"), 1), cos2=0.5),
                dict(axis=axis(float("inf"), 0, 1), cos2=0.5)):
        assert rn(**bad) == EINVAL, bad
    for required in ("points", "inlier", "plane", "header", "workspace"):
        assert rn(**{required: None}) == ENULL, required
    for k, by in (("points", 2), ("labels", 2), ("header", 2), ("plane", 4)):
        assert rn(**{k: odd(by)}) == EINVAL, k
    assert rn(workspace=odd(128)) == EINVAL and rn(workspace_bytes=need - 1) == EINVAL and rn(workspace_bytes=0) == EINVAL
    # the order: values (the axis among them), NULL, alignment and workspace
    assert rn(n=0, points=None) == EINVAL and rn(axis=axis(0, 0, 0), cos2=0.5, header=None) == EINVAL
    assert rn(plane=None, workspace_bytes=0) == ENULL and rn(inlier=None, points=odd(2)) == ENULL


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def _library_must_not_be_reached(pn2, monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pn2.plane, "launch", fail)
    monkeypatch.setattr(pn2.plane, "_on_device", fail)
    monkeypatch.setattr(pn2.cluster, "_on_device", fail)  # (cluster._device_cloud puts the cloud on the device for both)


def test_wrapper_argument_errors(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)  # (torch's own asks for a device)
    pts = np.zeros((10, 3), dtype=np.float32)
    lab = np.zeros((10,), dtype=np.int32)
    sp, sps, sc = pn2.segment_plane, pn2.segment_planes, pn2.score_planes
    for thr in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, "wide", None):  # 1e39 is inf, 1e-50 is 0 as float32
        with pytest.raises(ValueError, match="distance_threshold"):
            sp(pts, thr)
        with pytest.raises(ValueError, match="distance_threshold"):
            sps(pts, thr, 3, 10)
        with pytest.raises(ValueError, match="distance_threshold"):
            sc(pts, np.zeros((2, 6)), thr)
    for kw, what in ((dict(trials=0), "trials"), (dict(trials=2 ** 20 + 1), "trials"), (dict(seed=-1), "seed"),
                     (dict(seed=2 ** 64), "seed"), (dict(classes=[1]), "classes without labels"), (dict(labels=lab[:9]), "labels"),
                     (dict(labels=lab.astype(np.float32)), "labels: integers"), (dict(labels=lab, classes=[3, -1]), "classes"),
                     (dict(axis=(0, 0, 1)), "axis without max_angle"), (dict(max_angle=10), "max_angle without axis"),
                     (dict(axis=(0, 0, 0), max_angle=10), "axis"), (dict(axis=(0, 1), max_angle=10), "axis"),
                     (dict(axis=(0, float("nan"), 1), max_angle=10), "axis"), (dict(axis=(0, 0, 1), max_angle=-1), "max_angle"),
                     (dict(axis=(0, 0, 1), max_angle=91), "max_angle"), (dict(axis=(0, 0, 1), max_angle=float("nan")), "max_angle")):
        with pytest.raises(ValueError, match=what):
            sp(pts, 0.5, **kw)
        with pytest.raises(ValueError, match=what):
            sps(pts, 0.5, 3, 10, **kw)
    for bad in (np.zeros((10, 4), dtype=np.float32), np.zeros((10,), dtype=np.float32), np.zeros((2, 5, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="points"):
            sp(bad, 0.5)
        with pytest.raises(ValueError, match="points"):
            sc(bad, np.zeros((2, 6)), 0.5)
    for kw, what in ((dict(max_planes=0, min_inliers=5), "max_planes"), (dict(max_planes=2, min_inliers=0), "min_inliers")):
        with pytest.raises(ValueError, match=what):
            sps(pts, 0.5, **kw)
    for bad in (np.zeros((2, 5)), np.zeros((6,)), np.zeros((2, 3, 6)), [[0.0] * 6] * 2, None,
                np.broadcast_to(np.zeros((1, 4)), (2 ** 24 + 1, 4))):  # a list of rows, nothing, more rows than one call takes
        with pytest.raises(ValueError, match="planes"):
            sc(pts, bad, 0.5)
    with pytest.raises(ValueError, match="labels"):
        sc(pts, np.zeros((2, 6)), 0.5, labels=lab[:4])


def test_wrapper_refuses_a_capturing_stream(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    pts = np.zeros((10, 3), dtype=np.float32)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.segment_plane(pts, 0.5)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.segment_planes(pts, 0.5, 2, 5)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.score_planes(pts, np.zeros((1, 6)), 0.5)


def test_kitti_methods_take_the_new_arguments(pn2):
    import inspect
    PI = pn2.kitti_predict.PredictInterpolator
    ground = inspect.signature(PI.ground_for_frame).parameters
    assert list(ground) == ["self", "file_data", "distance_threshold", "trials", "seed", "max_angle", "dense_labels", "classes"]
    assert (ground["trials"].default, ground["seed"].default, ground["max_angle"].default) == (1024, 0, 15.0)
    objects = inspect.signature(PI.objects_for_frame).parameters
    assert list(objects)[-1] == "exclude" and objects["exclude"].default is None
