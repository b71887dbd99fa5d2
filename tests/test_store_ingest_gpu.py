"""GPU tests of pn2_scene_ingest (csrc/pn2_store.hip) and SemanticDataset(ingest="device").

The raw entry point runs with every output in the middle of a larger, poisoned store (the rows in front of and behind its n
rows must keep their poison), its small outputs and its workspace between poisoned guards, and is compared bit for bit with
the numpy model of the rule (tests/store_ingest_ref.py).  The dataset built on the device is compared with the host-built one:
the resident store, its small tables and the batches sampled from it."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import store_ingest_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
PRE, POST = 5, 7  # rows of the larger store in front of / behind the scene's slice
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]  # the edges of one row per lane, 64 lanes, 256 per workgroup


def _poisoned(torch, dev, nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=dev)


def _run(pn2, dev, points, colors=None, labels=None, want_perm=True, want_colors=None):
    """one pn2_scene_ingest call in poisoned surroundings -> dict like the model's (arrays read back), after checking that
    nothing but rows [0, n) of each output was written and that no input changed"""
    import torch
    launch, ptr = pn2._lib.launch, pn2._lib.ptr
    n = len(points)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    d_p, d_c, d_l = t(points, np.float64), t(colors, np.float64), t(labels, np.int32)
    want_colors = colors is not None if want_colors is None else want_colors
    rows = PRE + n + POST
    store = {k: _poisoned(torch, dev, rows * w) for k, w in (("points", 24), ("colors", 12), ("labels", 1), ("perm", 4))}
    small = _poisoned(torch, dev, 8 * (4 + 2 + 4 + 9 + 4 + 1 + 4))  # guards of 4 words around zrange (2), hist (9), status (1)
    nbytes = ctypes.c_uint64(0)
    launch("pn2_scene_ingest_workspace_size", dev, n, ctypes.byref(nbytes), stream=False)
    ws_raw = _poisoned(torch, dev, int(nbytes.value) + 512)
    off = (-ws_raw.data_ptr()) % 256
    ws = ws_raw[off:off + int(nbytes.value)]
    sl = lambda k, w: store[k][PRE * w:(PRE + n) * w]  # noqa: E731
    launch("pn2_scene_ingest", dev, n, ptr(d_p), ptr(d_c), ptr(d_l), ptr(sl("points", 24)),
           ptr(sl("colors", 12)) if want_colors else None, ptr(sl("labels", 1)), ptr(sl("perm", 4)) if want_perm else None,
           ptr(small, 8 * 4), ptr(small, 8 * 10), ptr(small, 8 * 23), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in store.items()}
    for k, w in (("points", 24), ("colors", 12), ("labels", 1), ("perm", 4)):
        assert (host[k][:PRE * w] == POISON).all() and (host[k][(PRE + n) * w:] == POISON).all(), "%s: a neighbouring row" % k
    if not want_colors:
        assert (host["colors"] == POISON).all(), "colours written although colors == NULL"
    if not want_perm:
        assert (host["perm"] == POISON).all()
    sm = small.cpu().numpy()
    for a, b in ((0, 4), (6, 10), (19, 23), (24, 28)):
        assert (sm[8 * a:8 * b] == POISON).all(), "guard words %d..%d of the small outputs" % (a, b)
    assert (sm[8 * 23 + 4:8 * 24] == POISON).all(), "status is one int32"
    wr = ws_raw.cpu().numpy()
    assert (wr[:off] == POISON).all() and (wr[off + int(nbytes.value):] == POISON).all(), "workspace guards"
    for d, a, dt in ((d_p, points, np.float64), (d_c, colors, np.float64), (d_l, labels, np.int32)):
        if d is not None:
            assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a, dtype=dt).tobytes(), "an input changed"
    cut = lambda k, w, dt: host[k][PRE * w:(PRE + n) * w].view(dt)  # noqa: E731
    return dict(status=int(sm[8 * 23:8 * 23 + 4].view(np.int32)[0]), perm=cut("perm", 4, np.int32) if want_perm else None,
                points=cut("points", 24, np.float64).reshape(n, 3), labels=cut("labels", 1, np.uint8),
                colors=cut("colors", 12, np.float32).reshape(n, 3) if want_colors else None,
                zrange=sm[8 * 4:8 * 6].view(np.float64), hist=sm[8 * 10:8 * 19].view(np.int64))


def _same(got, want):
    """bit for bit, every output"""
    assert got["status"] == want["status"] == 0
    for k in ("perm", "points", "labels", "colors", "zrange", "hist"):
        if want[k] is None or got[k] is None:
            assert k in ("perm", "colors") and (k == "perm" or want[k] is got[k]), k
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def _random_scene(seed, n):
    """x distinct; colours whose float32 rounding is inexact; labels 0..9"""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.permutation(n) * 0.03125 - 11.0, rs.uniform(-5, 5, n), rs.normal(0, 2, n)], 1)
    return pts, rs.uniform(0, 1, (n, 3)), rs.randint(0, 10, n).astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_tie_free_scenes_at_the_edges_of_the_thread_mapping(pn2, cuda, n):
    p, c, l = _random_scene(n, n)
    got = _run(pn2, cuda, p, c, l)
    assert np.array_equal(got["perm"], np.argsort(p[:, 0]))  # no ties: any argsort
    _same(got, M.ingest(p, c, l))
    assert (got["colors"].astype(np.float64) != c[got["perm"]]).any()  # the rounding was not a no-op


def test_ties_that_straddle_workgroups_keep_their_input_order(pn2, cuda):
    p, c, l = _random_scene(11, 1025)
    p[:, 0] = np.random.RandomState(12).randint(0, 8, 1025) * 0.5 - 2.0
    got = _run(pn2, cuda, p, c, l)
    assert np.array_equal(got["perm"], np.argsort(p[:, 0], kind="stable"))
    _same(got, M.ingest(p, c, l))


def test_all_x_equal_is_the_identity(pn2, cuda):
    p, c, l = _random_scene(13, 300)
    p[:, 0] = 3.25
    got = _run(pn2, cuda, p, c, l)
    assert np.array_equal(got["perm"], np.arange(300))
    _same(got, M.ingest(p, c, l))


def test_signed_zeros_compare_equal_and_keep_their_sign(pn2, cuda):
    p, c, l = _random_scene(14, 500)
    rs = np.random.RandomState(15)
    zeros = rs.permutation(500)[:200]
    p[:, 0] += 0.0078125  # no other x is a zero
    p[zeros, 0] = np.where(rs.randint(0, 2, 200) == 1, -0.0, 0.0)
    p[rs.permutation(500)[:9], 2] = np.array([0.0, -0.0, 0.0] * 3)
    got = _run(pn2, cuda, p, c, l)
    want = M.ingest(p, c, l)
    assert np.array_equal(got["perm"], np.argsort(p[:, 0], kind="stable"))
    _same(got, want)
    at = np.flatnonzero(got["points"][:, 0] == 0.0)
    assert len(at) == 200 and 0 < np.signbit(got["points"][at, 0]).sum() < 200
    q = np.abs(p) + 1.0  # zeros of both signs as the whole z range
    q[:, 2] = np.where(rs.randint(0, 2, 500) == 1, -0.0, 0.0)
    got = _run(pn2, cuda, q, c, l)
    _same(got, M.ingest(q, c, l))
    assert np.signbit(got["zrange"]).tolist() == [True, False]


def test_negative_denormal_and_huge_values(pn2, cuda):
    p, c, l = _random_scene(16, 700)
    rs = np.random.RandomState(17)
    special = np.array([-1e300, 1e300, 1e-310, -1e-310, 2e-310, -2e-310, 5e-324, -5e-324, 2.2250738585072014e-308, -1.5, 1.5])
    for col in (0, 2):
        p[rs.permutation(700)[:len(special)], col] = special
    got = _run(pn2, cuda, p, c, l)
    assert np.array_equal(got["perm"], np.argsort(p[:, 0], kind="stable"))
    _same(got, M.ingest(p, c, l))
    assert got["zrange"].tolist() == [-1e300, 1e300] and got["points"][0, 0] == -1e300 and got["points"][-1, 0] == 1e300


@pytest.mark.parametrize("col, bad", [(0, np.nan), (0, np.inf), (2, np.nan), (1, -np.inf)])
def test_a_non_finite_coordinate_is_status_1(pn2, cuda, col, bad):
    p, c, l = _random_scene(18, 1025)
    p[777, col] = bad
    assert M.ingest(p, c, l)["status"] == 1
    assert _run(pn2, cuda, p, c, l)["status"] == 1  # (and nothing outside the scene's rows was written)


@pytest.mark.parametrize("bad", [-1, 256])
def test_a_label_outside_the_byte_is_status_2(pn2, cuda, bad):
    p, c, l = _random_scene(19, 600)
    l[599] = bad
    assert M.ingest(p, c, l)["status"] == 2
    assert _run(pn2, cuda, p, c, l)["status"] == 2
    p[0, 1] = np.nan  # both: the coordinates win
    assert _run(pn2, cuda, p, c, l)["status"] == 1


def test_labels_the_shared_last_bin_and_uncounted_labels(pn2, cuda):
    p, c, _ = _random_scene(20, 1000)
    l = (np.arange(1000) % 10).astype(np.int32)  # 0 .. 9, a hundred of each
    got = _run(pn2, cuda, p, c, l)
    _same(got, M.ingest(p, c, l))
    assert got["hist"].tolist() == [100] * 8 + [200]
    l[:50] = 200  # valid, counted nowhere
    l[50:60] = (255, 10, 11, 64, 128, 254, 99, 12, 100, 17)
    got = _run(pn2, cuda, p, c, l)
    _same(got, M.ingest(p, c, l))
    assert got["hist"].sum() == 940 and (got["labels"] == 200).sum() == 50


def test_without_labels_and_without_colours(pn2, cuda):
    p, c, l = _random_scene(21, 513)
    got = _run(pn2, cuda, p, c, None)
    _same(got, M.ingest(p, c, None))
    assert not got["labels"].any() and got["hist"].tolist() == [513] + [0] * 8
    got = _run(pn2, cuda, p, None, l)  # colors == NULL: nothing read, nothing written, with and without an out_colors
    _same(got, M.ingest(p, None, l))
    got = _run(pn2, cuda, p, None, l, want_colors=True)
    assert (got["colors"].view(np.uint8) == POISON).all()
    got = _run(pn2, cuda, p, None, None, want_perm=False)
    _same(got, M.ingest(p, None, None))


# ---- the dataset ------------------------------------------------------------------------------------------------------------
N, B = 256, 4


def _ds_scenes():
    out = []
    for k, n in enumerate((3000, 1700, 4100)):
        rs = np.random.RandomState(30 + k)
        # columns of 2 m x 2 m hold ~140 to ~340 points: both sides of N
        pts = np.stack([rs.permutation(n) * 0.001953125 - 3.0, rs.uniform(0, 6, n), np.abs(rs.normal(0, 1, n))], 1)
        pts = pts.astype(np.float32).astype(np.float64)  # what a .pcd holds (x stays distinct: multiples of 2^-9 below 2^4)
        cols = rs.randint(0, 256, (n, 3)) / 255.0          # 8-bit colours, as a .pcd holds them
        out.append((pts, rs.randint(0, 9, n).astype(np.int32), cols, "scene%d" % k))
    return out


def _make(pn2, dev, ingest, scenes=None, path="", **kw):
    return pn2.dataset.SemanticDataset(N, "train", True, 2.0, 2.0, path, device=dev, seed=9, scenes=scenes, ingest=ingest, **kw)


def _assert_same_store_and_batches(host, devd):
    import torch
    a, b = host._upload(B), devd._upload(B)
    for k in ("points", "colors", "labels", "offsets", "cdf", "zsize", "lw"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    for name in ("scene_counts", "scene_offsets", "scene_probas", "scene_cdf", "scene_z_size", "label_weights"):
        x, y = getattr(host, name), getattr(devd, name)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert host.max_chunks == devd.max_chunks and host.scene_names == devd.scene_names
    assert host.get_total_num_points() == devd.get_total_num_points() and host.get_num_batches(B) == devd.get_num_batches(B)
    for _ in range(2):  # equal seeds: the same stream of batches
        x, y = host.sample_batch_in_all_files(B), devd.sample_batch_in_all_files(B)
        host.check_last()
        devd.check_last()
        for u, v in zip(x, y):
            assert torch.equal(u, v)
        assert torch.equal(host.last_sel, devd.last_sel)
    for i in range(devd.num_scenes):  # the per-scene attributes: device views of the store, the host's values
        assert devd.scene_points[i].is_cuda and devd.scene_points[i].dtype == torch.float64
        assert devd.scene_labels[i].dtype == torch.uint8 and devd.scene_colors[i].dtype == torch.float32
        assert devd.scene_points[i].cpu().numpy().tobytes() == host.scene_points[i].tobytes()
        assert np.array_equal(devd.scene_labels[i].cpu().numpy(), host.scene_labels[i])
        assert devd.scene_colors[i].cpu().numpy().tobytes() == host.scene_colors[i].astype(np.float32).tobytes()
        assert devd.scene_points[i].data_ptr() == b["points"][int(devd.scene_offsets[i])].data_ptr()  # (no copy)


def test_the_device_built_store_is_the_host_built_one(pn2, cuda):
    scenes = _ds_scenes()
    _assert_same_store_and_batches(_make(pn2, cuda, "host", scenes), _make(pn2, cuda, "device", scenes))


def test_device_tensors_of_other_dtypes_and_the_kept_permutation(pn2, cuda):
    import torch
    scenes = _ds_scenes()
    on = [(torch.from_numpy(p.astype(np.float32)).to(cuda), torch.from_numpy(l.astype(np.int64)).to(cuda),
           torch.from_numpy(c).to(cuda), name) for p, l, c, name in scenes]
    devd = _make(pn2, cuda, "device", on, keep_perm=True)
    _assert_same_store_and_batches(_make(pn2, cuda, "host", scenes), devd)
    for i, (p, l, c, _) in enumerate(scenes):
        perm = devd.scene_perm[i]
        assert perm.dtype == torch.int32 and perm.is_cuda
        perm = perm.cpu().numpy()
        assert np.array_equal(np.sort(perm), np.arange(len(p)))
        assert p[perm].tobytes() == devd.scene_points[i].cpu().numpy().tobytes()
        assert np.array_equal(l[perm], devd.scene_labels[i].cpu().numpy())
    # a batch's last_sel (store indices) back to the rows of the input
    devd.sample_batch_in_all_files(B, augment=False)
    devd.check_last()
    sel, scene = devd.last_sel.cpu().numpy(), devd.last_scene.cpu().numpy()
    for s in range(B):
        k = int(scene[s])
        rows = devd.scene_perm[k].cpu().numpy()[sel[s] - int(devd.scene_offsets[k])]
        assert scenes[k][0][rows].tobytes() == devd._upload(B)["points"].cpu().numpy()[sel[s]].tobytes()


def test_without_colour_and_without_labels(pn2, cuda):
    scenes = [(p, None, None, name) for p, _, _, name in _ds_scenes()]
    mk = lambda ingest: pn2.dataset.SemanticDataset(N, "test", False, 2.0, 2.0, "", device=cuda, seed=3, scenes=scenes,  # noqa: E731
                                                    ingest=ingest)
    host, devd = mk("host"), mk("device")
    a, b = host._upload(B), devd._upload(B)
    assert a["colors"] is None and b["colors"] is None and devd.scene_colors == [None] * 3
    for k in ("points", "labels", "offsets", "cdf", "zsize", "lw"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    import torch
    for u, v in zip(host.sample_batch_in_all_files(B), devd.sample_batch_in_all_files(B)):
        assert torch.equal(u, v)


def test_from_scene_files(pn2, cuda, tmp_path):
    scenes = _ds_scenes()
    for p, l, c, name in scenes:
        pn2.scene_io.write_point_cloud_pcd(str(tmp_path / (name + ".pcd")), p, c)
        pn2.scene_io.write_labels(str(tmp_path / (name + ".labels")), l)
    splits = {"train": [s[3] for s in scenes]}
    host = _make(pn2, cuda, "host", path=str(tmp_path), splits=splits)
    devd = _make(pn2, cuda, "device", path=str(tmp_path), splits=splits)
    _assert_same_store_and_batches(host, devd)
    assert devd.get_file_paths_without_ext() == host.get_file_paths_without_ext()


def test_the_wrapper_raises_on_the_statuses(pn2, cuda):
    p, l, c, name = _ds_scenes()[0]
    q = p.copy()
    q[5, 2] = np.nan
    with pytest.raises(ValueError, match="'scene0'.*non-finite coordinate"):
        _make(pn2, cuda, "device", [(q, l, c, name)])
    for bad in (-1, 256, 2 ** 31 + 3):
        k = l.astype(np.int64)
        k[7] = bad
        with pytest.raises(ValueError, match=r"labels must lie in \[0, 255\]"):
            _make(pn2, cuda, "device", [(p, k, c, name)])
    with pytest.raises(ValueError, match="must match"):
        _make(pn2, cuda, "device", [(p, l[:-1], c, name)])
    with pytest.raises(ValueError, match="no points"):
        _make(pn2, cuda, "device", [(p[:0], l[:0], c[:0], name)])
