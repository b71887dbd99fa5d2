"""The record kernels and their Python callers on the device (csrc/pn2_records.hip, scene_io.py) against the host model
tests/record_ref.py and the host readers / writers of util/point_cloud_util.py.  Every output sits inside a poisoned, guarded
buffer and everything is compared as bytes.  Both forms of each kernel run: the staged one (flags 0, where the stride allows
it) and the plain one (PN2_REC_FORM_PLAIN)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_ref as R  # noqa: E402
import scene_io_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON, GUARD = 0xA5, 256
BIG, PLAIN = 1, 2  # PN2_REC_BIG_ENDIAN, PN2_REC_FORM_PLAIN
FORMS = (0, PLAIN)
INVALID_START = 1000


def guarded(pn2, cuda, nbytes):
    buf = pn2.preprocess._aligned(GUARD + nbytes + GUARD, cuda)
    buf.fill_(POISON)
    return buf


def payload(buf, nbytes, what):
    """the bytes between the guards of a guarded buffer; the guards must still be poison"""
    got = buf.cpu().numpy().tobytes()
    assert got[:GUARD] == bytes([POISON]) * GUARD, "%s: a byte in front of the output" % what
    assert got[GUARD + nbytes:] == bytes([POISON]) * (len(got) - GUARD - nbytes), "%s: a byte behind the output" % what
    return got[GUARD:GUARD + nbytes]


def on_device(pn2, cuda, raw, room):
    """raw in a 16-byte aligned device buffer of exactly `room` bytes"""
    buf = pn2.preprocess._aligned(room, cuda)
    buf.fill_(POISON)
    buf[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    return buf


def run_unpack(pn2, cuda, raw, n, stride, offsets, types, kind, flags, want_colors, want_labels):
    """pn2_record_unpack on rows that end at n * stride rounded up to 16 (the read bound) -> the bytes of points, colors and
    labels (b"" where not asked for: the whole buffer is still poison) and what was added to the invalid counter, which starts
    at INVALID_START between two guard words"""
    L = pn2._lib
    rows = on_device(pn2, cuda, raw, (n * stride + 15) // 16 * 16)
    points, colors, labels = guarded(pn2, cuda, n * 24), guarded(pn2, cuda, n * 24), guarded(pn2, cuda, n * 4)
    counter = torch.tensor([-7, INVALID_START, -9], dtype=torch.int64, device=cuda)
    L.launch("pn2_record_unpack", cuda, L.ptr(rows), n, stride, L.int_array(offsets), L.int_array(types), kind, flags,
             L.ptr(points, GUARD), L.ptr(colors, GUARD) if want_colors else None, L.ptr(labels, GUARD) if want_labels else None,
             L.ptr(counter, 8))
    c = counter.tolist()
    assert c[0] == -7 and c[2] == -9
    return (payload(points, n * 24, "points"), payload(colors, n * 24 if want_colors else 0, "colors"),
            payload(labels, n * 4 if want_labels else 0, "labels"), c[1] - INVALID_START)


def check_unpack(pn2, cuda, raw, n, stride, offsets, types, kind, big=False, combos=None):
    """both forms against the model, with colours and labels asked for and not (an output not asked for stays poison)"""
    has_l = offsets[6] >= 0
    for want_colors, want_labels in (combos or [(c, l) for c in (True, False) for l in ((True, False) if has_l else (False,))]):
        want_p, want_c, want_l, want_bad = R.unpack(raw, n, stride, offsets, types, kind, big, want_colors, want_labels)
        for form in FORMS:
            got_p, got_c, got_l, got_bad = run_unpack(pn2, cuda, raw, n, stride, offsets, types, kind, form | (BIG if big else 0),
                                                      want_colors, want_labels)
            where = (n, stride, big, form, want_colors, want_labels)
            assert got_p == want_p.tobytes(), where
            assert got_c == (want_c.tobytes() if want_colors else b""), where
            assert got_l == (want_l.tobytes() if want_labels else b""), where
            assert got_bad == want_bad, where


@pytest.mark.parametrize("case", range(len(R.stride_cases())))
def test_unpack_strides(pn2, cuda, case):
    stride, offsets, types, kind = R.stride_cases()[case]
    for n in R.NS:
        check_unpack(pn2, cuda, R.case_rows(n, stride, offsets, types, seed=n), n, stride, offsets, types, kind)


def type_layouts(t):
    """the type code t in every slot it is legal in: once with every field at an odd offset of an odd stride, once with every
    field at a multiple of 8 in rows of 64 bytes (the reads of the field's own size)"""
    size, channel = R.SIZES[t], t in (R.U8, R.U16, R.F32, R.F64)
    for step, first, stride in ((size + 2 if size % 2 == 0 else size + 1, 1, None), (8, 0, 64)):
        at = [first + step * k for k in range(7)]
        if stride is None:
            stride = at[6] + size + (0 if (at[6] + size) % 2 else 1)
        offsets = at[:3] + (at[3:6] if channel else [-1] * 3) + [at[6]]
        yield stride, offsets, [t] * 7, R.THREE if channel else R.NONE


@pytest.mark.parametrize("t", range(8))
def test_unpack_every_type_in_every_slot(pn2, cuda, t):
    n = 300  # every byte value in every colour channel, every edge of edge_data
    for stride, offsets, types, kind in type_layouts(t):
        assert all(o % 2 == 1 for o in offsets if o >= 0) != (stride == 64)
        for big in (False, True):
            raw = R.case_rows(n, stride, offsets, types, big, seed=t)
            if t in (R.U8, R.I8):
                rec = np.frombuffer(raw, np.uint8).reshape(n, stride)
                assert all(len(set(rec[:, o].tolist())) == 256 for o in offsets if o >= 0)
            check_unpack(pn2, cuda, raw, n, stride, offsets, types, kind, big)


@pytest.mark.parametrize("t", [R.F32, R.F64])
def test_float_labels(pn2, cuda, t):
    """integral values, the two ends of int32 and the first values past them, fractions, NaN and infinities: the labels and the
    count of the invalid ones are the model's, and the count is added to a counter that does not start at zero"""
    values = [0.0, -0.0, 1.0, -1.0, 255.0, 2.0 ** 31 - 128, -2.0 ** 31, 2.0 ** 31, -2.0 ** 31 - 1, -2.0 ** 31 - 1024, 0.5, -1.5,
              np.nan, np.inf, -np.inf, 1e10, 2.0 ** -140, 16777216.0]
    n = 300
    data = np.resize(np.array(values, dtype=R.NUMPY[t]), n)
    offsets, types = R.slots_of(x=(0, R.F32), y=(4, R.F32), z=(8, R.F32), label=(13, t))
    stride = 13 + R.SIZES[t]
    for big in (False, True):
        raw = R.make_rows(n, stride, [(13, t, data)] + [(4 * k, R.F32, np.arange(n, dtype=np.float32)) for k in range(3)], big, seed=3)
        want = R.unpack(raw, n, stride, offsets, types, R.NONE, big, want_labels=True)
        ok = [0, 0, 1, -1, 255, 2 ** 31 - 128, -2 ** 31, 0, (-2 ** 31 if t == R.F32 else 0), 0, 0, 0, 0, 0, 0, 0, 0, 16777216]
        assert want[2][:len(values)].tolist() == ok and 0 < want[3] < n  # the model itself, against the rule written out
        check_unpack(pn2, cuda, raw, n, stride, offsets, types, R.NONE, big, combos=[(True, True), (False, True)])


def test_unpack_packed_colour_against_the_host_pcd_reader(pn2, cuda, tmp_path):
    """SIZE 8 8 8 4: double coordinates and PCD's rgb word"""
    U = pn2.util.point_cloud_util
    name, data, stride, offsets, types, kind = R.general_pcd_files(777)[0]
    assert (stride, kind) == (28, R.PACKED)
    path = str(tmp_path / "f64.pcd")
    with open(path, "wb") as f:
        f.write(data)
    want_p, want_c = U.read_point_cloud_pcd(path)
    for form in FORMS:
        got_p, got_c, _, _ = run_unpack(pn2, cuda, data[-777 * stride:], 777, stride, offsets, types, kind, form, True, False)
        assert got_p == want_p.tobytes() and got_c == want_c.tobytes()


def test_unpack_across_many_workgroups(pn2, cuda):
    """70 001 rows of 27 bytes: more than 256 workgroups; rows start at every residue modulo 16"""
    stride, offsets, types, kind = R.stride_cases()[4]
    assert stride == 27
    n = 70001
    check_unpack(pn2, cuda, R.case_rows(n, stride, offsets, types, seed=5), n, stride, offsets, types, kind, combos=[(True, False)])


def run_pack(pn2, cuda, points, colors, labels, coord, form):
    L = pn2._lib
    n, stride = len(points), R.pack_stride(coord, colors is not None, labels is not None)
    t = lambda a: None if a is None else torch.from_numpy(a).to(cuda)  # noqa: E731
    dp, dc, dl = t(points), t(colors), t(labels)
    rows = guarded(pn2, cuda, n * stride)
    kinds = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2}
    L.launch("pn2_record_pack", cuda, L.ptr(dp), kinds[points.dtype], L.ptr(dc), 0 if colors is None else kinds[colors.dtype],
             L.ptr(dl), n, R.F32 if coord == "float" else R.F64, form, L.ptr(rows, GUARD))
    for d, a in ((dp, points), (dc, colors), (dl, labels)):
        assert d is None or d.cpu().numpy().tobytes() == a.tobytes(), "an input changed"
    return payload(rows, n * stride, "rows")


def check_pack(pn2, cuda, n, layout):
    coord, has_c, has_l = layout
    p64, p32, c64, u8, labels = R.ply_inputs(n, seed=n)
    for points in (p64, p32):
        for colors in ((c64, u8) if has_c else (None,)):
            want = R.pack(points, colors, labels if has_l else None, coord)
            for form in FORMS:
                got = run_pack(pn2, cuda, points, colors, labels if has_l else None, coord, form)
                assert got == want, (n, layout, points.dtype, None if colors is None else colors.dtype, form)


@pytest.mark.parametrize("layout", R.PACK_LAYOUTS)
def test_pack_layouts(pn2, cuda, layout):
    for n in R.NS:
        check_pack(pn2, cuda, n, layout)


def test_pack_across_many_workgroups(pn2, cuda):
    for layout in (("double", True, False), ("float", True, True)):  # 27 and 19 bytes
        check_pack(pn2, cuda, 70001, layout)


def test_a_row_above_the_widest_stride_is_refused(pn2, cuda, tmp_path):
    assert R.stride_cases()[-1][0] == pn2.scene_io.MAX_REC_STRIDE == 1024
    head = R.pcd_head(["x", "y", "z", "more"], [8, 8, 8, 1], "FFFU", [1, 1, 1, 1001], 0)
    path = str(tmp_path / "wide.pcd")
    with open(path, "wb") as f:
        f.write(head)
    with pytest.raises(ValueError, match="1025 bytes"):
        pn2.read_point_cloud_pcd(path, cuda)


# ---- files -----------------------------------------------------------------------------------------------------------------
def as_bits(a):
    return a.cpu().numpy().tobytes() if torch.is_tensor(a) else np.ascontiguousarray(a).tobytes()


def same_arrays(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.is_cuda and str(g.dtype).split(".")[1] == str(w.dtype) and tuple(g.shape) == w.shape
        assert as_bits(g) == as_bits(w)


def test_ply_writer_and_reader(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    n = 1025
    p64, p32, c64, u8, labels = R.ply_inputs(n)
    want_path, got_path = str(tmp_path / "want.ply"), str(tmp_path / "got.ply")
    t = lambda a: None if a is None else torch.from_numpy(a).to(cuda)  # noqa: E731
    for coord, has_c, has_l in R.PACK_LAYOUTS:
        for points, colors in ((p64, c64), (p32, u8)):
            colors, lab = colors if has_c else None, labels if has_l else None
            U.write_point_cloud_ply(want_path, points, colors, lab, coord)
            with open(want_path, "rb") as f:
                want = f.read()
            for args, kw in (((t(points), t(colors), t(lab)), {}), ((points, colors, lab), {}),
                             ((t(points), t(colors), t(lab)), dict(chunk_rows=300))):
                pn2.write_point_cloud_ply(got_path, *args, coord=coord, **kw)
                with open(got_path, "rb") as f:
                    assert f.read() == want, (coord, has_c, has_l, kw)
            for kw in ({}, dict(chunk_rows=300)):
                same_arrays(pn2.read_point_cloud_ply(got_path, cuda, want_labels=has_l, **kw), U.read_point_cloud_ply(want_path, has_l))
            got = pn2.read_point_cloud_ply(got_path, cuda, want_colors=False, chunk_rows=300)
            assert got[1] is None and as_bits(got[0]) == as_bits(U.read_point_cloud_ply(want_path)[0])
    with pytest.raises(ValueError, match="label"):
        pn2.read_point_cloud_ply(got_path, cuda, want_labels=True, label_property="nothing")


def test_ply_of_nothing(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    want_path, got_path = str(tmp_path / "want.ply"), str(tmp_path / "got.ply")
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=cuda)  # noqa: E731
    U.write_point_cloud_ply(want_path, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), "double")
    pn2.write_point_cloud_ply(got_path, z((0, 3), torch.float64), z((0, 3), torch.float64), z((0,), torch.int32), coord="double")
    with open(want_path, "rb") as a, open(got_path, "rb") as b:
        assert a.read() == b.read() == U.ply_header(0, "double", True, True).encode()
    p, c, l = pn2.read_point_cloud_ply(got_path, cuda, want_labels=True)
    assert tuple(p.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(l.shape) == (0,) and l.dtype == torch.int32


def test_ply_reader_big_endian_ascii_and_truncated(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    n = 777
    stride, offsets, types, kind = R.stride_cases()[7]  # 64-byte rows: short x, uint y, double z, float colours, a double label
    props = {2: "short x", 8: "uint y", 16: "double z", 28: "float red", 32: "float green", 36: "float blue", 48: "double label"}
    lines, at = [], 0
    while at < stride:
        lines.append("property " + props.get(at, "uchar pad%d" % at))
        at += {"short": 2, "uint": 4, "float": 4, "double": 8, "uchar": 1}[lines[-1].split()[1]]
    path = str(tmp_path / "be.ply")
    for big in (True, False):
        rows = R.case_rows(n, stride, offsets, types, big, seed=9)
        head = "ply\nformat binary_%s_endian 1.0\nelement vertex %d\n%s\nend_header\n" % (("little", "big")[big], n, "\n".join(lines))
        with open(path, "wb") as f:
            f.write(head.encode() + rows)
        for kw in ({}, dict(chunk_rows=300)):
            same_arrays(pn2.read_point_cloud_ply(path, cuda, want_labels=True, **kw), U.read_point_cloud_ply(path, True))
    with open(path, "wb") as f:
        f.write(head.encode() + rows[:-5])
    with pytest.raises(ValueError, match="truncated"):
        pn2.read_point_cloud_ply(path, cuda)
    text = ("ply\nformat ascii 1.0\ncomment by hand\nelement vertex 2\nproperty double x\nproperty float y\nproperty short z\n"
            "property uchar red\nproperty ushort green\nproperty float blue\nproperty float class\nend_header\n"
            "0.1 0.1 -7 255 65535 0.25 3\n1e-320 1e-45 32767 0 1 nan 2.5\n")
    path = str(tmp_path / "a.ply")
    with open(path, "wb") as f:
        f.write(text.encode())
    same_arrays(pn2.read_point_cloud_ply(path, cuda, want_labels=True), U.read_point_cloud_ply(path, True))
    assert pn2.read_point_cloud_ply(path, cuda, want_colors=False)[1] is None


def test_read_point_cloud_dispatches_on_the_extension(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    p64, p32, c64, u8, labels = R.ply_inputs(300)
    for name, writer in (("a.pcd", U.write_point_cloud_pcd), ("b.PCD", U.write_point_cloud_pcd), ("c.ply", U.write_point_cloud_ply),
                         ("d.Ply", U.write_point_cloud_ply)):
        path = str(tmp_path / name)
        writer(path, p32, u8 / 255.0)
        same_arrays(pn2.read_point_cloud(path, cuda), U.read_point_cloud(path))
        assert pn2.read_point_cloud(path, cuda, want_colors=False, chunk_rows=100)[1] is None
    same_arrays(pn2.read_point_cloud(str(tmp_path / "c.ply"), cuda), U.read_point_cloud_ply(str(tmp_path / "c.ply")))
    with pytest.raises(ValueError, match="pcd or .ply"):
        pn2.read_point_cloud(str(tmp_path / "e.xyz"), cuda)


def launches(pn2, fn):
    lib = pn2._lib.lib
    lib.trace = calls = []
    try:
        out = fn()
    finally:
        lib.trace = None
    return out, [c[0] for c in calls]


def test_pcd_reader_picks_the_kernel_by_the_layout(pn2, cuda, tmp_path):
    """the general-layout files read equal to the host model through pn2_record_unpack; a file of 4-byte fields still goes
    through pn2_pcd_unpack"""
    U = pn2.util.point_cloud_util
    for name, data, stride, offsets, types, kind in R.general_pcd_files(777):
        path = str(tmp_path / (name + ".pcd"))
        with open(path, "wb") as f:
            f.write(data)
        want = U.read_point_cloud_pcd(path)
        for kw in ({}, dict(chunk_rows=300)):
            got, names = launches(pn2, lambda: pn2.read_point_cloud_pcd(path, cuda, **kw))
            same_arrays(got, want)
            assert names == ["pn2_record_unpack"] * (3 if kw else 1)
        assert pn2.read_point_cloud_pcd(path, cuda, want_colors=False)[1] is None
    path = str(tmp_path / "words.pcd")
    rows = np.random.RandomState(2).randint(0, 2 ** 32, (777, 5), dtype=np.uint64).astype(np.uint32)
    with open(path, "wb") as f:
        f.write(S.pcd_bytes(["x", "y", "z", "intensity", "rgb"], rows))
    got, names = launches(pn2, lambda: pn2.read_point_cloud_pcd(path, cuda, chunk_rows=300))
    same_arrays(got, U.read_point_cloud_pcd(path))
    assert names == ["pn2_pcd_unpack"] * 3


# ---- the dataset and the example ------------------------------------------------------------------------------------------------
def test_dataset_from_ply_scenes_is_the_dataset_from_pcd_scenes(pn2, cuda, tmp_path):
    N, B = 256, 4
    scenes = []
    for k, n in enumerate((3000, 1700)):
        rs = np.random.RandomState(40 + k)
        pts = np.stack([rs.permutation(n) * 0.001953125 - 3.0, rs.uniform(0, 6, n), np.abs(rs.normal(0, 1, n))], 1).astype(np.float32)
        scenes.append((pts, rs.randint(0, 9, n).astype(np.int32), rs.randint(0, 256, (n, 3)).astype(np.uint8), "scene%d" % k))
    pcd_dir, ply_dir = tmp_path / "pcd", tmp_path / "ply"
    for d in (pcd_dir, ply_dir):
        d.mkdir()
    for p, l, c, name in scenes:
        pn2.write_point_cloud_pcd(str(pcd_dir / (name + ".pcd")), p, c)
        pn2.write_point_cloud_ply(str(ply_dir / (name + ".ply")), p, c, coord="float")  # the same float32 values
        for d in (pcd_dir, ply_dir):
            pn2.write_labels(str(d / (name + ".labels")), l)
    splits = {"train": [s[3] for s in scenes]}
    mk = lambda d, ingest: pn2.dataset.SemanticDataset(N, "train", True, 2.0, 2.0, str(d), device=cuda, seed=9, splits=splits,  # noqa: E731
                                                       ingest=ingest)
    stores = [mk(d, ingest)._upload(B) for ingest in ("host", "device") for d in (pcd_dir, ply_dir)]
    for other in stores[1:]:
        for k in ("points", "colors", "labels", "offsets", "cdf", "zsize", "lw"):
            assert stores[0][k].dtype == other[k].dtype and as_bits(stores[0][k]) == as_bits(other[k]), k
    one = pn2.dataset.semantic_dataset.SemanticFileData(str(ply_dir / "scene0"), device=cuda)  # <prefix>.ply where there is no .pcd
    two = pn2.dataset.semantic_dataset.SemanticFileData(str(pcd_dir / "scene0"), device=cuda)
    assert torch.equal(one.points, two.points) and torch.equal(one.colors, two.colors) and torch.equal(one.labels, two.labels)


@pytest.mark.timeout(300)
def test_example_writes_ply_files_that_read_back(pn2, cuda, tmp_path):
    """examples/predict_semantic3d.py --format ply on one synthetic scene: the .ply files hold what the .labels beside them were
    voted from -- the sparse cloud reads back to the example's float32 points, the dense cloud to the scene and the label colours"""
    U = pn2.util.point_cloud_util
    N, samples, scene_points = 512, 3, 20000
    cmd = [sys.executable, os.path.join(ROOT, "examples", "predict_semantic3d.py"), "--num_samples", str(samples), "--batch-size", "4",
           "--points", str(N), "--npoint", "256,64,32,16", "--scenes", "1", "--scene-points", str(scene_points), "--voxel", "0.1",
           "--format", "ply"]
    run = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    sparse, dense = tmp_path / "result" / "sparse", tmp_path / "result" / "dense"
    name = "syn_validation_0"
    assert not list(sparse.glob("*.pcd")) and not list(dense.glob("*.pcd"))
    sp, sc = pn2.read_point_cloud(str(sparse / (name + ".ply")), cuda)
    same_arrays((sp, sc), U.read_point_cloud_ply(str(sparse / (name + ".ply"))))
    sl = U.load_labels(str(sparse / (name + ".labels")))
    assert tuple(sp.shape) == (samples * N, 3) and sl.shape == (samples * N,) and not bool(sc.any())
    dp, dc = pn2.read_point_cloud(str(dense / (name + "_colored.ply")), cuda)
    dl = U.load_labels(str(dense / (name + ".labels")))
    assert tuple(dp.shape) == (scene_points, 3) and dl.shape == (scene_points,)
    f32 = lambda a: a.cpu().numpy().astype(np.float32)  # noqa: E731
    lab, col = pn2.predict.label_dense(f32(sp), sl, f32(dp))  # the arrays that were written
    assert np.array_equal(lab.cpu().numpy(), dl)
    assert as_bits(dc) == as_bits(col.cpu().numpy().astype(np.float64) / 255.0)
