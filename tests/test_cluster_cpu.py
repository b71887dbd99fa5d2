"""CPU tests of Euclidean clustering (csrc/pn2_cluster.hip, cluster.py): the numpy model of the rules (tests/cluster_ref.py) against
scipy's connected components and against hand-made cases with written-out answers, the header's prototypes and the binding, the
refusals of the entry points with placeholder pointers, the wrapper's argument errors and its refusal of a capturing stream.
Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_ref as C  # noqa: E402

ARGS = {
    "pn2_cluster_workspace_size": ("n", "bytes"),
    "pn2_cluster_points": ("n", "points", "labels", "eps", "min_points", "max_points", "ids", "header", "workspace",
                           "workspace_bytes", "stream"),
    "pn2_cluster_stats": ("n", "nclusters", "points", "labels", "ids", "first", "size", "label", "bbox", "stream"),
    "pn2_cluster_colors": ("n", "ids", "rgb", "stream"),
}


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,eps,with_labels", [(500, 0.08, False), (1500, 0.06, True), (300, 0.3, True), (64, 0.01, False)])
def test_model_against_scipy(n, eps, with_labels):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rs = np.random.RandomState(n)
    pts = rs.random_sample((n, 3)).astype(np.float32)
    labels = rs.randint(-1, 3, n).astype(np.int32) if with_labels else None
    pts[n // 3, 1] = np.nan
    pts[n // 2, 0] = np.inf
    ids, header = C.cluster(pts, eps, labels)
    ok = C.valid_mask(pts, labels)
    pairs = C.edges(pts, eps, labels)
    assert ok[pairs].all()
    g = sparse.coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    ncomp, comp = connected_components(g, directed=False)
    assert header[2] == ncomp - (~ok).sum() == header[1] and header[3] == ok.sum() == header[4]
    assert (ids[~ok] == -1).all() and (ids[ok] >= 0).all()
    # the same partition, and numbered by ascending first index
    for a, b in ((ids[ok], comp[ok]), (comp[ok], ids[ok])):
        assert len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist()))
    firsts = [np.nonzero(ids == c)[0][0] for c in range(header[1])]
    assert firsts == sorted(firsts)


def test_model_on_hand_made_cases():
    z = np.zeros
    # 0-1-2 chained along x in steps of exactly eps; 3 alone; 4 non-finite; 5 within eps of 3 but of another label
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [1.0, 0, 0], [5, 5, 5], [np.nan, 0, 0], [5, 5.25, 5]], dtype=np.float32)
    ids, header = C.cluster(pts, 0.5)
    assert ids.tolist() == [0, 0, 0, 1, -1, 1] and header.tolist() == [0, 2, 2, 5, 5, 0, 0, 0]
    labels = np.array([2, 2, 2, 7, 7, 1], dtype=np.int32)
    ids, header = C.cluster(pts, 0.5, labels)
    assert ids.tolist() == [0, 0, 0, 1, -1, 2] and header.tolist() == [0, 3, 3, 5, 5, 0, 0, 0]
    first, size, label, bbox = C.stats(pts, ids, labels)
    assert first.tolist() == [0, 3, 5] and size.tolist() == [3, 1, 1] and label.tolist() == [2, 7, 1]
    assert bbox.tolist() == [[0, 0, 0, 1, 0, 0], [5, 5, 5, 5, 5, 5], [5, 5.25, 5, 5, 5.25, 5]]
    # label -1 takes the middle of the chain out: two singletons are left of it
    ids, header = C.cluster(pts, 0.5, np.array([2, -1, 2, 7, 7, 1], dtype=np.int32))
    assert ids.tolist() == [0, -1, 1, 2, -1, 3] and header.tolist() == [0, 4, 4, 4, 4, 0, 0, 0]
    # the size filter renumbers what is left, in the order of the first index
    ids, header = C.cluster(pts, 0.5, min_points=2)
    assert ids.tolist() == [0, 0, 0, 1, -1, 1] and header.tolist() == [0, 2, 2, 5, 5, 0, 0, 0]
    ids, header = C.cluster(pts, 0.5, min_points=3)
    assert ids.tolist() == [0, 0, 0, -1, -1, -1] and header.tolist() == [0, 1, 2, 5, 3, 0, 0, 0]
    ids, header = C.cluster(pts, 0.5, min_points=1, max_points=2)
    assert ids.tolist() == [-1, -1, -1, 0, -1, 0] and header.tolist() == [0, 1, 2, 5, 2, 0, 0, 0]
    ids, header = C.cluster(pts, 0.5, min_points=4)
    assert ids.tolist() == [-1] * 6 and header.tolist() == [0, 0, 2, 5, 0, 0, 0, 0]
    # the threshold is inclusive, and one ulp beyond it is outside
    pair = z((2, 3), dtype=np.float32)
    pair[1, 0] = 0.5
    assert C.cluster(pair, 0.5)[0].tolist() == [0, 0]
    pair[1, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    assert C.cluster(pair, 0.5)[0].tolist() == [0, 1]
    # the box orders -0.0 below +0.0
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0]], dtype=np.float32)
    bbox = C.stats(zeros, np.zeros(2, dtype=np.int32))[3]
    assert np.signbit(bbox[0]).tolist() == [True, True, False, False, False, False]


def test_model_chain_needs_few_rounds():
    rs = np.random.RandomState(5)
    n = 4097
    order = rs.permutation(n)
    pts = np.zeros((n, 3), dtype=np.float32)
    pts[order, 0] = np.arange(n) * 0.5 - 1000.25
    low, rounds = C.components(n, C.edges(pts, 0.5))
    assert (low == 0).all() and rounds <= 20


def test_model_colors():
    ids = np.array([-1, 0, 1, 2, 1000, 2 ** 31 - 1], dtype=np.int32)
    rgb = C.colors(ids)
    assert rgb[0].tolist() == list(C.GREY) and rgb[1].tolist() == [255, 0, 0]  # id 0 hashes to 0: hue 0
    for row in rgb[1:].tolist():  # full saturation: one channel 255, one 0
        assert max(row) == 255 and min(row) == 0
    # by hand, in python integers
    for i, want in zip(ids[1:].tolist(), rgb[1:].tolist()):
        h = (i * 0x9E3779B1) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x85EBCA77) & 0xFFFFFFFF
        h ^= h >> 13
        s, f = (h % 1536) >> 8, (h % 1536) & 255
        assert want == [[255, f, 0], [255 - f, 255, 0], [0, 255, f], [0, 255 - f, 255], [f, 0, 255], [255, 0, 255 - f]][s]
    assert len({tuple(r) for r in C.colors(np.arange(64)).tolist()}) >= 60  # neighbouring ids look different


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS and name not in pn2._lib._STATEFUL
    i, f, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_cluster_points"].argtypes == [i, p, p, f, i, i, p, p, p, z, p]
    assert fns["pn2_cluster_stats"].argtypes == [i, i, p, p, p, p, p, p, p, p]
    assert fns["pn2_cluster_colors"].argtypes == [i, p, p, p]
    assert fns["pn2_cluster_workspace_size"].argtypes == [i, p]
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_cluster.hip" in pn2._lib._build.SOURCES
    with open(os.path.join(ROOT, "open3d-pointnet2-semantic3d_amd", "csrc", "pn2_cluster.hip")) as src:
        assert "pn2_grid_knn.h" not in src.read()  # its own grid
    assert pn2.cluster.STATUS_NAMES[1] and pn2.euclidean_clusters is pn2.cluster.euclidean_clusters


def _workspace_bytes(pn2, n):
    nbytes = ctypes.c_ulonglong(0)
    assert pn2._lib.lib.pn2_cluster_workspace_size(n, ctypes.byref(nbytes)) == 0
    return int(nbytes.value)


def test_workspace_size(pn2):
    K = pn2._lib.ABI.constants
    query = pn2._lib.lib.pn2_cluster_workspace_size
    nbytes = ctypes.c_ulonglong(7)
    assert query(0, ctypes.byref(nbytes)) == K["PN2_EINVAL"] and query(-4, ctypes.byref(nbytes)) == K["PN2_EINVAL"]
    assert query(100, None) == K["PN2_ENULL"] and nbytes.value == 7
    size = lambda n: _workspace_bytes(pn2, n)  # noqa: E731
    # nine per-point arrays of 4 + 4 + 8 + 8 + 16 + 4 * 4 = 56 bytes a point, each rounded up to 256, and the sort's share
    # (small clouds only: the sort sizes a large one from the device's properties)
    assert size(1) >= 9 * 256 and size(1000) >= 56 * 1000 and size(1000) <= size(1001) < 400 * 1000


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
    n = 1000
    need = _workspace_bytes(pn2, n)
    pts = _caller(pn2, "pn2_cluster_points", dict(n=n, points=fake, labels=fake, eps=0.5, min_points=1, max_points=0, ids=fake,
                                                  header=fake, workspace=fake, workspace_bytes=need, stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                dict(min_points=0), dict(min_points=-2), dict(max_points=-1)):
        assert pts(**bad) == EINVAL, bad
    for required in ("points", "ids", "header", "workspace"):
        assert pts(**{required: None}) == ENULL, required
    for k in ("points", "labels", "ids", "header"):
        assert pts(**{k: odd(2)}) == EINVAL, k
    assert pts(workspace=odd(128)) == EINVAL and pts(workspace_bytes=need - 1) == EINVAL and pts(workspace_bytes=0) == EINVAL
    # the order: sizes, NULL, alignment and workspace
    assert pts(n=0, points=None) == EINVAL and pts(ids=None, workspace_bytes=0) == ENULL

    st = _caller(pn2, "pn2_cluster_stats", dict(n=n, nclusters=10, points=fake, labels=fake, ids=fake, first=fake, size=fake,
                                                label=fake, bbox=fake, stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(nclusters=0), dict(nclusters=-1)):
        assert st(**bad) == EINVAL, bad
    assert st(nclusters=n + 1) == ERANGE
    for required in ("points", "ids", "first", "size", "label", "bbox"):
        assert st(**{required: None}) == ENULL, required
    for k in ("points", "labels", "ids", "first", "size", "label", "bbox"):
        assert st(**{k: odd(2)}) == EINVAL, k
    assert st(n=0, nclusters=5, ids=None) == EINVAL and st(nclusters=n + 1, ids=None) == ERANGE and st(ids=None, bbox=odd(1)) == ENULL

    col = _caller(pn2, "pn2_cluster_colors", dict(n=n, ids=fake, rgb=fake, stream=None))
    assert col(n=0) == EINVAL and col(n=-7) == EINVAL
    assert col(ids=None) == ENULL and col(rgb=None) == ENULL and col(ids=odd(1)) == EINVAL
    assert col(n=0, ids=None) == EINVAL and col(rgb=None, ids=odd(2)) == ENULL


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
    lab =np.zeros((10,), dtype=np.int32)
    ec = pn2.cluster.euclidean_clusters
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, "wide", None):  # 1e39 is inf, 1e-50 is 0 as float32
        with pytest.raises(ValueError, match="eps"):
            ec(pts, eps)
    for kw, what in ((dict(min_points=0), "min_points"), (dict(min_points=-3), "min_points"), (dict(max_points=-1), "max_points"),
                     (dict(min_points=5, max_points=4), "max_points below"), (dict(classes=[1]), "classes without labels"),
                     (dict(labels=lab[:9]), "labels"), (dict(labels=lab.astype(np.float32)), "labels: integers"),
                     (dict(labels=lab, classes=[3, -1]), "classes")):
        with pytest.raises(ValueError, match=what):
            ec(pts, 0.5, **kw)
    for bad in (np.zeros((10, 4), dtype=np.float32), np.zeros((10,), dtype=np.float32), np.zeros((2, 5, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="points"):
            ec(bad, 0.5)
    with pytest.raises(ValueError, match="MI355X only"):  # a host tensor: there is no CPU path
        pn2.cluster.cluster_colors(torch.zeros(4, dtype=torch.int32))


def test_wrapper_refuses_a_capturing_stream(pn2, monkeypatch):
    import torch
    _library_must_not_be_reached(pn2, monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        pn2.cluster.euclidean_clusters(np.zeros((10, 3), dtype=np.float32), 0.5)
    with pytest.raises(RuntimeError, match="capturing"):  # before the arguments are looked at
        pn2.cluster.euclidean_clusters(np.zeros((10, 4), dtype=np.float32), -1.0)
