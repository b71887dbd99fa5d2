"""CPU tests around pn2_scene_ingest (csrc/pn2_store.hip) and SemanticDataset(ingest="device"): the numpy model of the rule
(tests/store_ingest_ref.py) is tied to the host constructor that is already trusted, the header declares the entry points, and
every argument error is refused on the host.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import store_ingest_ref as M  # noqa: E402


def _scene(seed, n, ties=False):
    """points float64 (x distinct unless ties), labels int32 in 0..9, colours float64 whose float32 rounding is inexact"""
    rs = np.random.RandomState(seed)
    if ties:
        x = rs.randint(0, 8, n) * 0.25
    else:
        x = rs.permutation(n) * 0.03125 - 7.0  # distinct, exact, in random order
    pts = np.stack([x, rs.uniform(-5, 5, n), rs.normal(0, 2, n)], 1)
    return pts, rs.randint(0, 10, n).astype(np.int32), rs.uniform(0, 1, (n, 3))


def _host(pn2, scenes, split="train", use_color=True):
    return pn2.dataset.SemanticDataset(64, split, use_color, 2.0, 2.0, "", device="cpu", scenes=scenes)


def test_model_equals_the_host_constructor_on_tie_free_scenes(pn2):
    raw = [_scene(s, n) for s, n in ((1, 700), (2, 1), (3, 257))]
    ds = _host(pn2, [(p, l, c, "s%d" % i) for i, (p, l, c) in enumerate(raw)])
    hists = []
    for i, (p, l, c) in enumerate(raw):
        m = M.ingest(p, c, l)
        assert m["status"] == 0
        assert m["points"].tobytes() == ds.scene_points[i].tobytes()
        assert np.array_equal(m["labels"], ds.scene_labels[i]) and m["labels"].dtype == np.uint8
        assert m["colors"].tobytes() == ds.scene_colors[i].astype(np.float32).tobytes()
        assert np.float64(m["zrange"][1] - m["zrange"][0]).tobytes() == np.float64(ds.scene_z_size[i]).tobytes()
        hists.append(m["hist"])
    lw = pn2.dataset.multi_scene.label_weights_from_counts(hists)
    assert lw.dtype == ds.label_weights.dtype and lw.tobytes() == ds.label_weights.tobytes()
    assert lw.tobytes() == pn2.dataset.multi_scene.label_weights_of([l for _, l, _ in raw]).tobytes()


def test_model_without_labels_and_colours(pn2):
    p, _, _ = _scene(4, 300)
    ds = _host(pn2, [(p, None, None, "s")], split="test")
    m = M.ingest(p)
    assert m["points"].tobytes() == ds.scene_points[0].tobytes() and m["colors"] is None
    assert not m["labels"].any() and m["hist"].tolist() == [300] + [0] * 8


def test_model_on_ties_keeps_the_sorted_column_and_the_rows(pn2):
    p, l, c = _scene(5, 1025, ties=True)
    ds = _host(pn2, [(p, l, c, "s")])
    m = M.ingest(p, c, l)
    assert np.array_equal(m["points"][:, 0], ds.scene_points[0][:, 0])
    rows = lambda pts, lab, col: sorted(zip(map(bytes, np.ascontiguousarray(pts)), lab.tolist(),  # noqa: E731
                                            map(bytes, np.ascontiguousarray(col.astype(np.float32)))))
    assert rows(m["points"], m["labels"], m["colors"]) == rows(ds.scene_points[0], ds.scene_labels[0], ds.scene_colors[0])
    # ... and ties keep their input order
    assert all(a < b for a, b in zip(m["perm"][:-1], m["perm"][1:]) if p[a, 0] == p[b, 0])


def test_model_statuses_and_signed_zeros():
    p, l, c = _scene(6, 40)
    for col, bad in ((0, np.nan), (0, np.inf), (2, np.nan), (1, -np.inf)):
        q = p.copy()
        q[17, col] = bad
        assert M.ingest(q, c, l)["status"] == 1
    for bad in (-1, 256):
        k = l.copy()
        k[3] = bad
        assert M.ingest(p, c, k)["status"] == 2
        q = p.copy()
        q[0, 1] = np.nan
        assert M.ingest(q, c, k)["status"] == 1  # both: the coordinates win
    k = l.copy()
    k[:3] = (200, 9, 8)
    m = M.ingest(p, c, k)
    assert m["status"] == 0 and m["hist"].sum() == 39 and m["hist"][8] == (k == 8).sum() + (k == 9).sum()
    q = p.copy()
    q[:4, 0] = (0.0, -0.0, -0.0, 0.0)
    q[4:, 0] = np.abs(q[4:, 0]) + 1.0
    q[:, 2] = np.abs(q[:, 2]) + 1.0
    q[5:7, 2] = (0.0, -0.0)
    m = M.ingest(q, c, l)
    assert m["perm"][:4].tolist() == [0, 1, 2, 3] and np.signbit(m["points"][:4, 0]).tolist() == [False, True, True, False]
    assert np.signbit(m["zrange"][0]) and m["zrange"][0] == 0.0


def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert fns["pn2_scene_ingest_workspace_size"].restype is i
    assert fns["pn2_scene_ingest_workspace_size"].argtypes == [i, p]
    assert fns["pn2_scene_ingest"].restype is i and fns["pn2_scene_ingest"].argtypes == [i] + [p] * 11 + [z, p]
    assert fns["pn2_scene_ingest"].argnames == ("n", "points", "colors", "labels", "out_points", "out_colors", "out_labels",
                                                "out_perm", "out_zrange", "out_hist", "status", "workspace", "workspace_bytes",
                                                "stream")
    assert {"pn2_scene_ingest", "pn2_scene_ingest_workspace_size"} <= set(pn2._lib.SIGNATURES)
    assert "pn2_scene_ingest" not in pn2._lib._TRACE_ARGS and "pn2_scene_ingest" not in pn2._lib._STATEFUL


def test_argument_errors_are_refused_without_a_gpu(pn2):
    L = pn2._lib.lib
    EINVAL, ENULL = pn2._lib.ABI.constants["PN2_EINVAL"], pn2._lib.ABI.constants["PN2_ENULL"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    names = pn2._lib.ABI.functions["pn2_scene_ingest"].argnames
    good = dict(n=1000, points=fake, colors=fake, labels=fake, out_points=fake, out_colors=fake, out_labels=fake, out_perm=fake,
                out_zrange=fake, out_hist=fake, status=fake, workspace=fake, workspace_bytes=0, stream=None)

    def call(**change):
        a = dict(good, **change)
        return L.pn2_scene_ingest(*[a[k] for k in names])

    assert call() == EINVAL                                   # the workspace is too small
    assert call(workspace_bytes=4096) == EINVAL               # (less than the keys alone: no device is asked anything)
    assert call(n=0) == EINVAL and call(n=-5) == EINVAL
    for required in ("points", "out_points", "out_labels", "out_zrange", "out_hist", "status", "workspace"):
        assert call(**{required: None}) == ENULL, required
    assert call(out_colors=None) == ENULL                     # colours given, nowhere to put them
    assert call(out_colors=None, colors=None) == EINVAL       # fine up to the workspace
    assert call(labels=None, out_perm=None) == EINVAL
    assert call(n=0, points=None) == EINVAL                   # the count is looked at first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)            # noqa: E731
    big = 1 << 40
    for name, k in (("points", 4), ("out_points", 4), ("out_zrange", 4), ("out_hist", 4), ("out_colors", 2), ("labels", 1),
                    ("status", 2), ("workspace", 128)):
        assert call(workspace_bytes=big, **{name: odd(k)}) == EINVAL, name
    nbytes = ctypes.c_uint64(0)
    assert L.pn2_scene_ingest_workspace_size(0, ctypes.byref(nbytes)) == EINVAL
    assert L.pn2_scene_ingest_workspace_size(100, None) == ENULL


def test_device_ingest_refuses_the_cpu(pn2):
    p, l, c = _scene(7, 50)
    with pytest.raises(ValueError, match="MI355X"):
        pn2.dataset.SemanticDataset(64, "train", True, 2.0, 2.0, "", device="cpu", scenes=[(p, l, c, "s")], ingest="device")
    with pytest.raises(ValueError, match="ingest"):
        _ = pn2.dataset.SemanticDataset(64, "train", True, 2.0, 2.0, "", device="cpu", scenes=[(p, l, c, "s")], ingest="gpu")
    with pytest.raises(ValueError, match="keep_perm"):
        _ = pn2.dataset.SemanticDataset(64, "train", True, 2.0, 2.0, "", device="cpu", scenes=[(p, l, c, "s")], keep_perm=True)
    ds = pn2.dataset.SemanticDataset(64, "train", True, 2.0, 2.0, "", device="cpu", scenes=[(p, l, c, "s")], ingest="host")
    assert ds.ingest == "host" and isinstance(ds.scene_points[0], np.ndarray) and ds.get_total_num_points() == 50
