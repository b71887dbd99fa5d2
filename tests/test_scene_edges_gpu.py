"""GPU tests of csrc/pn2_scene.hip at its edges, every comparison exact (np.array_equal): the kernels promise float64, the same
operations in the same order as the reference, so no tolerance enters.  The model is oracle/dataset_oracle.py
(voxel_down_sample; FileDataOracle._extract_z_box, _center_box, the repeat branch of _get_fix_sized_sample_mask); the inputs come
from tests/scene_edge_cases.py, and test_scene_edges_cpu.py asserts from the model alone that each edge named below occurs.

A. pn2_voxel_downsample through downsample.down_sample_arrays
  A1 coordinates on voxel faces (p = origin + (j - 0.5) vs): thousands of quotients that are exact integers, that fall below j,
     that a multiplication with 1 / vs or a float32 quotient would put into another voxel; vs = 0.25 is the exact control.
  A2 one voxel of 3001 members over ten decades: any order of summation but the input's gives another mean; again with 20000
     members beside 5000 single-member voxels (one thread walks a voxel).
  A3 n = 1, 2 (one point twice), 255 .. 257, 1023 .. 1025, and 262143 .. 262145 across the 1024-workgroup cap of the min / max pass.
  A4 voxels differing only in iz, only in iy, only in ix, and ix = iy = iz = 2^21 - 1 (bit 62 of the key): sorted by (ix, iy, iz).
  A5 an extent whose largest index is 2^21 - 1 succeeds exactly, 2^21 raises, per axis.
  A6 label ties go to the smaller label, label 63 is counted, 64 and -1 raise, labels=None / colors=None.
  A7 a minimum of -0.0, subnormal coordinates and colours (compared bit for bit, signs of zero included).
  A8 float32 points, a strided view, int64 labels.
  A9 a NaN, +inf or -inf coordinate in the first, a middle or the last row raises ValueError (status 3).
  A10 nothing left (all labels 0, or no rows): empty tensors, nothing launched.
  A11 the entry point: a workspace one byte short or misaligned is PN2_EINVAL; out_colors / out_labels may be NULL.
B. pn2_scene_extract_z_box / pn2_scene_sample through dataset.SemanticFileData, centres and masks given
  B1 lattice scene: x == cx + 5 outside; x == cx - 5, y == cy +- 5, z == cz +- scene_z_size inside.
  B2 the centre at sorted index 0 and n - 1 of a 700-point scene.   B3 x-slabs of 1023, 1024, 1025, 3000 rows, half inside.
  B4 cnt in {1, 2, npts - 1, npts, npts + 1, 3 npts + 7} for npts in {5, 1024, 1500}.   B5 capacity == cnt and cnt - 1.
  B6 masks selecting npts - 1 / npts + 1, bytes of 255, bytes past cnt.   B7 rejected samples come back zero, check_last() and
  strict raise.   B8 a scene 1e5 m from the origin.   B9 no labels / no colours, at construction and as NULL pointers.

The rejections are defined outcomes: no call below makes a kernel read or write out of range."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_edge_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, cuda):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ======================================================================================================================
# A. voxel down-sampling
# ======================================================================================================================
def _down(pn2, cuda, pts, cols, labels, vs, **kw):
    import torch
    sp, sc, sl = pn2.downsample.down_sample_arrays(_t(pts, cuda), _t(cols, cuda), _t(labels, cuda), voxel_size=vs, **kw)
    assert sp.dtype == torch.float64 and sc.dtype == torch.float64 and (sl is None or sl.dtype == torch.int32)
    return sp.cpu().numpy(), sc.cpu().numpy(), None if sl is None else sl.cpu().numpy()


def _same(got, want, what="", bits=False):
    """points, colours, labels of the device against the model's, exactly; bits: the sign of a zero counts too"""
    for name, g, w in zip(("points", "colors", "labels"), got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))
        if bits and g.dtype == np.float64:
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), (what, name)


def _check(pn2, cuda, pts, cols, labels, vs, what="", bits=False, **kw):
    got = _down(pn2, cuda, pts, cols, labels, vs, **kw)
    _same(got, C.voxel_model(pts, cols, labels, vs, **kw), what, bits)
    return got


@pytest.mark.parametrize("origin", C.FACE_ORIGINS)
@pytest.mark.parametrize("vs", C.FACE_VS)
def test_a1_voxel_faces(pn2, cuda, vs, origin):
    pts, _, cols, labels = C.face_cloud(vs, origin)
    _check(pn2, cuda, pts, cols, labels, vs)


def test_a2_sum_in_input_order(pn2, cuda):
    pts, cols, labels = C.sum_order_cloud(C.SUM_MEMBERS)
    got = _check(pn2, cuda, pts, cols, labels, 1.0)
    assert len(got[0]) == 1


def test_a2_sum_in_input_order_beside_single_member_voxels(pn2, cuda):
    pts, cols, labels = C.sum_order_cloud(C.SUM_MEMBERS_WIDE, C.SUM_SINGLES)
    got = _check(pn2, cuda, pts, cols, labels, 1.0)
    assert len(got[0]) == 1 + C.SUM_SINGLES


@pytest.mark.parametrize("n", C.COUNTS_SMALL + C.COUNTS_LARGE)
def test_a3_counts(pn2, cuda, n):
    pts, cols, labels = C.count_cloud(n)
    _check(pn2, cuda, pts, cols, labels, C.COUNT_VS)


def test_a4_output_sorted_by_ix_iy_iz(pn2, cuda):
    pts, cols, labels, _ = C.order_cloud()
    sp = _check(pn2, cuda, pts, cols, labels, C.ORDER_VS)[0]
    out = np.floor((sp - (pts.min(axis=0) - C.ORDER_VS * 0.5)) / C.ORDER_VS).astype(np.int64)
    assert [tuple(v) for v in out.tolist()] == sorted(C.ORDER_INDICES)


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a5_the_21_bit_limit(pn2, cuda, axis):
    pts, cols, labels = C.limit_cloud(axis, C.EXTENT_FITS)
    got = _check(pn2, cuda, pts, cols, labels, C.LIMIT_VS)
    assert len(got[0]) == 2
    pts, cols, labels = C.limit_cloud(axis, C.EXTENT_OVER)
    with pytest.raises(ValueError) as err:
        _down(pn2, cuda, pts, cols, labels, C.LIMIT_VS)
    assert pn2.downsample.STATUS_NAMES[1] in str(err.value)


def test_a6_labels(pn2, cuda):
    pts, cols, labels = C.label_cloud()
    got = _check(pn2, cuda, pts, cols, labels, C.LABEL_VS)
    assert got[2].tolist() == [3, 63, 8, 2]  # the tie between 3 and 5 goes to 3; 63 is counted
    assert _check(pn2, cuda, pts, cols, None, C.LABEL_VS)[2] is None
    sc = _check(pn2, cuda, pts, None, labels, C.LABEL_VS)[1]
    assert sc.shape == (4, 3) and not sc.any()
    for bad, kw in ((64, {}), (-1, {}), (-1, dict(skip_label_zero=False)), (64, dict(skip_label_zero=False))):
        wrong = labels.copy()
        wrong[5] = bad
        with pytest.raises(ValueError) as err:
            _down(pn2, cuda, pts, cols, wrong, C.LABEL_VS, **kw)
        assert pn2.downsample.STATUS_NAMES[2] in str(err.value)
    # label 0 is a label like any other once it is not skipped
    zero = np.where(labels == 5, 0, labels).astype(np.int32)
    assert _check(pn2, cuda, pts, cols, zero, C.LABEL_VS, skip_label_zero=False)[2].tolist() == [0, 63, 8, 2]
    assert _check(pn2, cuda, pts, cols, zero, C.LABEL_VS)[2].tolist() == [3, 63, 8, 2]


def test_a7_signed_zero_and_subnormals(pn2, cuda):
    for cloud in (C.signed_zero_cloud, C.subnormal_cloud):
        pts, cols, labels = cloud()
        _check(pn2, cuda, pts, cols, labels, 0.05, cloud.__name__, bits=True)


def test_a8_input_forms(pn2, cuda):
    import torch
    pts, cols, labels = C.plain_cloud(2 * C.PLAIN_N)
    dn = pn2.downsample.down_sample_arrays
    host = lambda out: [None if t is None else t.cpu().numpy() for t in out]  # noqa: E731
    # float32 points: the result of their float64 copy
    p32 = pts.astype(np.float32)
    _same(host(dn(_t(p32, cuda), _t(cols, cuda), _t(labels, cuda), voxel_size=C.PLAIN_VS)),
          C.voxel_model(p32.astype(np.float64), cols, labels, C.PLAIN_VS), "float32 points")
    # strided views: the result of the dense copies
    tp, tc, tl = _t(pts, cuda), _t(cols, cuda), _t(labels, cuda)
    assert not tp[::2].is_contiguous()
    _same(host(dn(tp[::2], tc[::2], tl[::2], voxel_size=C.PLAIN_VS)), C.voxel_model(pts[::2], cols[::2], labels[::2], C.PLAIN_VS),
          "strided views")
    # int64 labels, float32 colours
    c32 = cols.astype(np.float32)
    got = dn(tp, _t(c32, cuda), tl.to(torch.int64), voxel_size=C.PLAIN_VS)
    assert got[2].dtype == torch.int32 and got[1].dtype == torch.float64
    _same(host(got), C.voxel_model(pts, c32.astype(np.float64), labels, C.PLAIN_VS), "int64 labels")


@pytest.mark.parametrize("row", C.NONFINITE_ROWS)
@pytest.mark.parametrize("value", C.NONFINITE_VALUES, ids=("nan", "+inf", "-inf"))
def test_a9_non_finite_coordinates_are_refused(pn2, cuda, value, row):
    pts, cols, labels = C.plain_cloud()
    for axis in range(3):
        bad = pts.copy()
        bad[row, axis] = value
        out = None
        with pytest.raises(ValueError) as err:
            out = _down(pn2, cuda, bad, cols, labels, C.PLAIN_VS)
        assert out is None and pn2.downsample.STATUS_NAMES[3] in str(err.value), (axis, str(err.value))
    _check(pn2, cuda, pts, cols, labels, C.PLAIN_VS)  # and the next call is an ordinary one


def test_a10_nothing_left(pn2, cuda):
    import torch
    pts, cols, labels = C.plain_cloud()
    dn = pn2.downsample.down_sample_arrays

    def empty(out, with_labels=True):
        sp, sc, sl = out
        assert sp.shape == (0, 3) and sp.dtype == torch.float64 and sp.is_cuda
        assert sc.shape == (0, 3) and sc.dtype == torch.float64 and sc.is_cuda
        if with_labels:
            assert sl.shape == (0,) and sl.dtype == torch.int32 and sl.is_cuda
        else:
            assert sl is None

    calls = []
    real = pn2.downsample.launch
    pn2.downsample.launch = lambda *a, **k: calls.append(a[0]) or real(*a, **k)
    try:
        empty(dn(_t(pts, cuda), _t(cols, cuda), _t(np.zeros_like(labels), cuda)))            # every label 0
        empty(dn(_t(pts, cuda), None, _t(np.zeros_like(labels), cuda)))
        empty(dn(_t(pts[:0], cuda), _t(cols[:0], cuda), _t(labels[:0], cuda)))                # no rows
        empty(dn(_t(pts[:0], cuda), _t(cols[:0], cuda), _t(labels[:0], cuda), skip_label_zero=False))
        empty(dn(_t(pts[:0], cuda), None, None), with_labels=False)
        assert calls == []  # nothing was launched
        dn(_t(pts, cuda), _t(cols, cuda), _t(labels, cuda))
        assert calls == ["pn2_voxel_downsample"]
    finally:
        pn2.downsample.launch = real


def _raw_voxel(pn2, cuda, pts, cols, labels, vs, short=0, shift=0, out_colors=True, out_labels=True):
    """one raw call of pn2_voxel_downsample: the workspace `short` bytes too small / `shift` bytes off its 256-byte alignment"""
    import torch
    L = pn2._lib
    n = len(pts)
    p, c, l = _t(pts, cuda), _t(cols, cuda), _t(labels, cuda)
    out_p = torch.full((n, 3), -7.0, dtype=torch.float64, device=cuda)
    out_c = torch.full((n, 3), -7.0, dtype=torch.float64, device=cuda)
    out_l = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    count = torch.zeros((1,), dtype=torch.int32, device=cuda)
    status = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    need = L.lib.pn2_voxel_downsample_workspace_bytes(n)
    ws = torch.empty((need + 512,), dtype=torch.uint8, device=cuda)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256 + shift
    with torch.cuda.device(cuda):
        rc = L.lib.pn2_voxel_downsample(n, L.ptr(p), L.ptr(c), L.ptr(l), float(vs), L.ptr(out_p), L.ptr(out_c) if out_colors else None,
                                        L.ptr(out_l) if out_labels else None, L.ptr(count), L.ptr(status), base, need - short,
                                        L.stream_ptr())
    torch.cuda.synchronize()
    m = int(count.item())
    return rc, int(status.item()), out_p.cpu().numpy(), out_c.cpu().numpy(), out_l.cpu().numpy(), m


def test_a11_the_entry_point(pn2, cuda):
    einval = pn2._lib.ABI.constants["PN2_EINVAL"]
    pts, cols, labels = C.plain_cloud()
    want = C.voxel_model(pts, cols, labels, C.PLAIN_VS)
    rc, st, op, oc, ol, m = _raw_voxel(pn2, cuda, pts, cols, labels, C.PLAIN_VS)
    assert (rc, st, m) == (0, 0, len(want[0]))
    _same((op[:m], oc[:m], ol[:m]), want, "raw call")
    assert (op[m:] == -7).all() and (oc[m:] == -7).all() and (ol[m:] == -7).all()  # nothing past the voxels is written
    for kw in (dict(short=1), dict(shift=1), dict(shift=128)):
        rc, st, op, oc, ol, m = _raw_voxel(pn2, cuda, pts, cols, labels, C.PLAIN_VS, **kw)
        assert rc == einval and st == -7 and m == 0 and (op == -7).all(), kw  # refused before anything ran
    rc, st, op, oc, ol, m = _raw_voxel(pn2, cuda, pts, cols, labels, C.PLAIN_VS, out_colors=False, out_labels=False)
    assert (rc, st, m) == (0, 0, len(want[0])) and np.array_equal(op[:m], want[0])
    assert (oc == -7).all() and (ol == -7).all()
    rc, st, op, oc, ol, m = _raw_voxel(pn2, cuda, pts, None, None, C.PLAIN_VS)
    assert (rc, st, m) == (0, 0, len(want[0])) and np.array_equal(op[:m], want[0]) and not oc[:m].any() and (ol == -7).all()


# ======================================================================================================================
# B. the single-scene sampler
# ======================================================================================================================
FIELDS = ("centered", "raw", "labels", "colors")
DTYPES = dict(centered=np.float32, raw=np.float64, labels=np.int32, colors=np.float32, sel=np.int32)


def _fd(pn2, cuda, scene, **kw):
    pts, labels, cols = scene
    return pn2.dataset.SemanticFileData(points=pts, labels=labels, colors=cols, box_size_x=C.BOX, box_size_y=C.BOX, device=cuda, **kw)


def _batch(fd, cuda, centers, masks, npts, cap):
    """the index lists of the columns, then the batch -> host arrays"""
    import torch
    ci = torch.from_numpy(np.asarray(centers, dtype=np.int64)).to(cuda)
    idx, cnt = fd.extract_z_box(fd.points[ci], cap)
    out = fd.sample_batch(len(centers), npts, center_indices=ci, sample_masks=_t(masks, cuda), capacity=cap)
    got = dict(zip(FIELDS, (t.cpu().numpy() for t in out)))
    got.update(idx=idx.cpu().numpy(), cnt=cnt.cpu().numpy(), status=fd.last_status.cpu().numpy(), sel=fd.last_sel.cpu().numpy())
    assert np.array_equal(got["cnt"], fd.last_cnt.cpu().numpy())
    return got


def _check_sample(got, s, m, cap, what=""):
    assert got["status"][s] == 0, (what, s, got["status"])
    assert got["cnt"][s] == m["cnt"], (what, s)
    assert got["idx"].dtype == np.int32 and np.array_equal(got["idx"][s, :min(m["cnt"], cap)], m["idx"][:cap]), (what, s)
    for k in FIELDS + ("sel",):
        assert got[k].dtype == DTYPES[k] and np.array_equal(got[k][s], m[k]), (what, s, k)


def _check_rejected(got, s, status):
    assert got["status"][s] == status
    for k in FIELDS:
        assert not got[k][s].any(), (s, k)  # zero-filled, as the class promises


def _check_batch(pn2, cuda, scene, centers, masks, npts, cap, what=""):
    o, fd = C.oracle_of(scene), _fd(pn2, cuda, scene)
    got = _batch(fd, cuda, centers, masks, npts, cap)
    for s, ci in enumerate(centers):
        _check_sample(got, s, C.sample_model(o, ci, masks[s], npts), cap, what)
    fd.check_last()
    return got


def test_b1_column_faces(pn2, cuda):
    scene = C.lattice_scene()
    o = C.oracle_of(scene)
    centers = [C.find_point(o, xyz) for xyz in C.LATTICE_CENTERS]
    cap = max(len(C.column(o, ci)) for ci in centers)
    _check_batch(pn2, cuda, scene, centers, C.random_masks(o, centers, C.LATTICE_NPTS, cap, 111), C.LATTICE_NPTS, cap)


def test_b2_ends_of_the_scene(pn2, cuda):
    scene = C.ends_scene()
    o = C.oracle_of(scene)
    centers = [0, C.ENDS_N - 1, C.ENDS_N // 2]
    _check_batch(pn2, cuda, scene, centers, C.random_masks(o, centers, C.ENDS_NPTS, C.ENDS_N, 121), C.ENDS_NPTS, C.ENDS_N)


def test_b3_slabs_across_the_workgroup_width(pn2, cuda):
    scene = C.chunk_scene()
    o = C.oracle_of(scene)
    centers = [C.block_center(o, k) for k in range(len(C.CHUNK_SLABS))]
    cap = max(len(C.column(o, ci)) for ci in centers)
    got = _check_batch(pn2, cuda, scene, centers, C.random_masks(o, centers, C.CHUNK_NPTS, cap, 131), C.CHUNK_NPTS, cap)
    for s in range(len(centers)):
        assert (np.diff(got["idx"][s, :got["cnt"][s]]) > 0).all()  # scene order


@pytest.mark.parametrize("npts", C.COUNT_NPTS)
def test_b4_count_against_npts(pn2, cuda, npts):
    scene = C.count_scene(npts)
    centers, masks, cap = C.count_plan(C.oracle_of(scene), npts)
    got = _check_batch(pn2, cuda, scene, centers, masks, npts, cap)
    assert got["cnt"].tolist() == [1, 2, npts - 1, npts, npts + 1, npts + 1, npts + 1, 3 * npts + 7]


def _wide_plan(npts=1024):
    """the count scene of npts = 1024: its widest column (3079), the 1025 one, the 1023 one and the 2 one"""
    scene = C.count_scene(npts)
    o = C.oracle_of(scene)
    centers = [C.block_center(o, k) for k in (5, 4, 2, 1)]
    return scene, o, centers, npts, max(C.count_sizes(npts))


def test_b5_capacity(pn2, cuda):
    scene, o, centers, npts, widest = _wide_plan()
    masks = C.random_masks(o, centers, npts, widest, 151)
    _check_batch(pn2, cuda, scene, centers, masks, npts, widest, "capacity == cnt")
    fd = _fd(pn2, cuda, scene)
    cap = widest - 1
    got = _batch(fd, cuda, centers, np.ascontiguousarray(masks[:, :cap]), npts, cap)
    assert got["cnt"][0] == widest  # the count is reported in full, the list holds the first cap indices
    assert np.array_equal(got["idx"][0], C.column(o, centers[0])[:cap])
    _check_rejected(got, 0, 2)
    for s in (1, 2, 3):
        _check_sample(got, s, C.sample_model(o, centers[s], masks[s], npts), cap, "capacity == cnt - 1")
    with pytest.raises(RuntimeError):
        fd.check_last()


def test_b6_bad_masks(pn2, cuda):
    scene, o, centers, npts, cap = _wide_plan()
    good = C.random_masks(o, centers, npts, cap, 161)
    fd = _fd(pn2, cuda, scene)
    first_set, first_clear = int(np.flatnonzero(good[0])[0]), int(np.flatnonzero(good[0] == 0)[0])
    for at, value in ((first_set, 0), (first_clear, 1), (first_clear, 255)):  # npts - 1 and npts + 1 bytes set
        masks = good.copy()
        masks[0, at] = value
        got = _batch(fd, cuda, centers, masks, npts, cap)
        _check_rejected(got, 0, 3)
        for s in (1, 2, 3):
            _check_sample(got, s, C.sample_model(o, centers[s], good[s], npts), cap, "neighbour of a bad mask")
        with pytest.raises(RuntimeError):
            fd.check_last()
    # bytes of 255 count as set; bytes at positions >= cnt are ignored (also for columns that use no mask at all)
    masks = good * 255
    for s, ci in enumerate(centers):
        masks[s, len(C.column(o, ci)):] = (1, 255, 7)[s % 3]
    assert masks[1, 1025:].all() and masks[3, 2:].all() and not masks[0, cap:].size
    got = _batch(fd, cuda, centers, masks, npts, cap)
    for s in range(4):
        _check_sample(got, s, C.sample_model(o, centers[s], good[s], npts), cap, "bytes of 255 and bytes past cnt")
    fd.check_last()


def _raw_sample(pn2, fd, cuda, idx, cnt, masks, npts, labels=True, colors=True, fill=0):
    """one raw call of pn2_scene_sample on the scene of `fd`, outputs pre-filled with `fill` -> host arrays"""
    import torch
    L = pn2._lib
    b, cap = idx.shape
    out = dict(sel=torch.full((b, npts), fill, dtype=torch.int32, device=cuda),
               centered=torch.full((b, npts, 3), fill, dtype=torch.float32, device=cuda),
               raw=torch.full((b, npts, 3), fill, dtype=torch.float64, device=cuda),
               labels=torch.full((b, npts), fill, dtype=torch.int32, device=cuda),
               colors=torch.full((b, npts, 3), fill, dtype=torch.float32, device=cuda),
               status=torch.full((b,), -7, dtype=torch.int32, device=cuda))
    mask = _t(masks, cuda)
    L.launch("pn2_scene_sample", cuda, b, npts, cap, L.ptr(fd.points), L.ptr(fd.labels) if labels else None,
             L.ptr(fd.colors) if colors else None, L.ptr(idx), L.ptr(cnt), L.ptr(mask), C.HALF, C.HALF, L.ptr(out["sel"]),
             L.ptr(out["centered"]), L.ptr(out["raw"]), L.ptr(out["labels"]), L.ptr(out["colors"]), L.ptr(out["status"]))
    fd.last_status, fd.last_sel, fd.last_cnt = out["status"], out["sel"], cnt
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(idx=idx.cpu().numpy(), cnt=cnt.cpu().numpy())
    return got


def test_b7_rejected_samples(pn2, cuda):
    import torch
    scene, o, centers, npts, cap = _wide_plan()
    good = C.random_masks(o, centers, npts, cap, 171)
    fd = _fd(pn2, cuda, scene)
    # status 1: a centre outside the scene has an empty column (a centre that is a scene point never has)
    ci = torch.from_numpy(np.asarray(centers, dtype=np.int64)).to(cuda)
    pos = fd.points[ci].clone()
    pos[1, 0] = 1.0e6
    pos[3, 1] = -1.0e6
    idx, cnt = fd.extract_z_box(pos, cap)
    assert cnt.cpu().tolist() == [len(C.column(o, centers[0])), 0, len(C.column(o, centers[2])), 0]
    got = _raw_sample(pn2, fd, cuda, idx, cnt, good, npts)
    for s in (1, 3):
        _check_rejected(got, s, 1)
        assert not got["sel"][s].any()  # nothing of a rejected sample is written
    for s in (0, 2):
        _check_sample(got, s, C.sample_model(o, centers[s], good[s], npts), cap, "neighbour of an empty column")
    with pytest.raises(RuntimeError) as err:
        fd.check_last()
    assert "[0, 1, 0, 1]" in str(err.value)
    # the raw call on good columns is the class's batch
    idx, cnt = fd.extract_z_box(fd.points[ci], cap)
    got = _raw_sample(pn2, fd, cuda, idx, cnt, good, npts)
    for s, c in enumerate(centers):
        _check_sample(got, s, C.sample_model(o, c, good[s], npts), cap, "raw call")
    fd.check_last()
    # strict=True: sample_batch itself raises, for status 2 and for status 3; without a fault it returns the exact batch
    strict = _fd(pn2, cuda, scene, strict=True)
    _check_sample(_batch(strict, cuda, centers, good, npts, cap), 0, C.sample_model(o, centers[0], good[0], npts), cap, "strict")
    with pytest.raises(RuntimeError) as err:
        strict.sample_batch(4, npts, center_indices=ci, sample_masks=_t(np.ascontiguousarray(good[:, :cap - 1]), cuda), capacity=cap - 1)
    assert "[2, 0, 0, 0]" in str(err.value)
    holed = good.copy()
    holed[1, int(np.flatnonzero(holed[1])[-1])] = 0
    with pytest.raises(RuntimeError) as err:
        strict.sample_batch(4, npts, center_indices=ci, sample_masks=_t(holed, cuda), capacity=cap)
    assert "[0, 3, 0, 0]" in str(err.value)


def test_b8_centring_far_from_the_origin(pn2, cuda):
    scene = C.far_scene()
    o = C.oracle_of(scene)
    cap = len(o.points)
    _check_batch(pn2, cuda, scene, list(C.FAR_CENTERS), C.random_masks(o, C.FAR_CENTERS, C.FAR_NPTS, cap, 181), C.FAR_NPTS, cap)


def test_b9_without_labels_or_colours(pn2, cuda):
    pts, labels, cols = C.ends_scene()
    centers, npts, cap = [10, 350, 690], C.ENDS_NPTS, C.ENDS_N
    for scene in ((pts, None, cols), (pts, labels, None), (pts, None, None)):
        o = C.oracle_of(scene)
        got = _check_batch(pn2, cuda, scene, centers, C.random_masks(o, centers, npts, cap, 191), npts, cap)
        assert scene[1] is not None or not got["labels"].any()
        assert scene[2] is not None or not got["colors"].any()
    # use_color=False stores zeros too
    o = C.oracle_of((pts, labels, None))
    masks = C.random_masks(o, centers, npts, cap, 192)
    fd = _fd(pn2, cuda, (pts, labels, cols), use_color=False)
    got = _batch(fd, cuda, centers, masks, npts, cap)
    for s, ci in enumerate(centers):
        _check_sample(got, s, C.sample_model(o, ci, masks[s], npts), cap, "use_color=False")
    # NULL labels / colours in a raw call: zeros are WRITTEN (the outputs start at 7)
    import torch
    fd = _fd(pn2, cuda, (pts, labels, cols))
    idx, cnt = fd.extract_z_box(fd.points[torch.tensor(centers, device=cuda)], cap)
    got = _raw_sample(pn2, fd, cuda, idx, cnt, masks, npts, labels=False, colors=False, fill=7)
    o = C.oracle_of((pts, None, None))
    for s, ci in enumerate(centers):
        _check_sample(got, s, C.sample_model(o, ci, masks[s], npts), cap, "NULL labels and colours")
    assert not got["labels"].any() and not got["colors"].any()
