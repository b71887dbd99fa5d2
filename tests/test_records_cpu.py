"""CPU tests of the record kernels' surroundings (csrc/pn2_records.hip, scene_io.py, util/point_cloud_util.py): the PLY and
general PCD headers, the host readers and writers against the model tests/record_ref.py and against payloads made with
struct.pack, the binding, and the C ABI's refusals -- none needs a GPU."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_ref as R  # noqa: E402
import scene_io_ref as S  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


# ---- PLY headers ----------------------------------------------------------------------------------------------------------
def test_ply_header_text_is_exact(pn2):
    U = pn2.util.point_cloud_util
    assert U.ply_header(7, "float", False, False) == (
        "ply\nformat binary_little_endian 1.0\ncomment Created by pn2\nelement vertex 7\n"
        "property float x\nproperty float y\nproperty float z\nend_header\n")
    assert U.ply_header(0, "double", True, True) == (
        "ply\nformat binary_little_endian 1.0\ncomment Created by pn2\nelement vertex 0\n"
        "property double x\nproperty double y\nproperty double z\n"
        "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nend_header\n")
    with pytest.raises(ValueError):
        U.ply_header(1, "half", False, False)


def test_ply_headers_parse_back(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    for coord, has_c, has_l in R.PACK_LAYOUTS:
        path = write(tmp_path / "h.ply", U.ply_header(5, coord, has_c, has_l).encode() + b"payload")
        with open(path, "rb") as f:
            h = U.read_ply_header(f)
            assert f.read() == b"payload"  # left at the first payload byte
        size = 4 if coord == "float" else 8
        assert (h.format, h.n, h.stride) == ("binary_little_endian", 5, R.pack_stride(coord, has_c, has_l))
        offsets, types, kind = h.slots
        assert offsets[:3] == [0, size, 2 * size] and types[:3] == [R.F32 if coord == "float" else R.F64] * 3
        assert kind == (R.THREE if has_c else R.NONE) and offsets[3:6] == ([3 * size + k for k in range(3)] if has_c else [-1] * 3)
        assert offsets[6] == (3 * size + 3 * has_c if has_l else -1) and (not has_l or types[6] == R.I32)
    # both type spellings, comments and obj_info between the lines, a trailing face element with a list property
    text = ("ply\nformat binary_big_endian 1.0\ncomment one\nobj_info two\nelement vertex 3\nproperty int8 a\nproperty uint8 b\n"
            "comment three\nproperty int16 c\nproperty uint16 red\nproperty int32 x\nproperty uint32 e\nproperty float32 y\n"
            "property float64 z\nproperty char f\nproperty uchar g\nproperty short h\nproperty ushort green\nproperty int i\n"
            "property uint j\nproperty float scalar_label\nproperty double blue\nproperty int class\n"
            "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    with open(write(tmp_path / "t.ply", text.encode()), "rb") as f:
        h = U.read_ply_header(f)
    want = [R.I8, R.U8, R.I16, R.U16, R.I32, R.U32, R.F32, R.F64, R.I8, R.U8, R.I16, R.U16, R.I32, R.U32, R.F32, R.F64, R.I32]
    assert h.types == want and h.format == "binary_big_endian" and h.n == 3
    assert h.offsets == [int(o) for o in np.cumsum([0] + [R.SIZES[t] for t in want])[:-1]] and h.stride == sum(R.SIZES[t] for t in want)
    offsets, types, kind = h.slots
    at = dict(zip(h.names, h.offsets))
    assert offsets == [at["x"], at["y"], at["z"], at["red"], at["green"], at["blue"], at["class"]]  # class comes before scalar_label
    assert types == [R.I32, R.F32, R.F64, R.U16, R.U16, R.F64, R.I32] and kind == R.THREE
    with open(write(tmp_path / "t.ply", text.encode()), "rb") as f:
        offsets, types, _ = U.read_ply_header(f, label_property="scalar_label").slots
    assert offsets[6] == at["scalar_label"] and types[6] == R.F32


@pytest.mark.parametrize("text", [
    "plx\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
    "ply\nformat binary_little_endian 2.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
    "ply\nformat binary_middle_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n",
    "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n",                     # no z
    "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty half z\nend_header\n",    # unknown type
    "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
    "property list uchar int n\nend_header\n",                                                                     # a list in vertex
    "ply\nformat ascii 1.0\nelement face 1\nproperty list uchar int v\nelement vertex 1\nproperty float x\nproperty float y\n"
    "property float z\nend_header\n",                                                                              # vertex not first
    "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n",             # no end_header
    "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
    "property int red\nproperty int green\nproperty int blue\nend_header\n",                                       # int colours
])
def test_ply_headers_that_are_refused(pn2, tmp_path, text):
    with open(write(tmp_path / "bad.ply", text.encode()), "rb") as f:
        with pytest.raises(ValueError):
            pn2.util.point_cloud_util.read_ply_header(f)


def test_missing_label_property_is_refused(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    path = write(tmp_path / "a.ply", U.ply_header(0, "float", False, False).encode())
    with open(path, "rb") as f:
        with pytest.raises(ValueError):
            U.read_ply_header(f, label_property="mine")
    with pytest.raises(ValueError):
        U.read_point_cloud_ply(path, want_labels=True)


def test_a_hand_written_open3d_style_file(pn2, tmp_path):
    """The header below is written by hand from the layout Open3D's PLY writer uses (double coordinates, uchar colours); it was
    NOT produced by Open3D, which is not available to this suite.  The payload is made with struct.pack, independent of numpy."""
    U = pn2.util.point_cloud_util
    rows = [(1.5, -2.25, 1e-300, 0, 128, 255), (float("inf"), -0.0, 123456.789012345, 255, 1, 2), (3.0, 4.0, 5.0, 7, 8, 9)]
    head = ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex %d\nproperty double x\n"
            "property double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(rows))
    path = write(tmp_path / "o3d.ply", head.encode() + b"".join(struct.pack("<dddBBB", *r) for r in rows))
    points, colors = U.read_point_cloud_ply(path)
    assert bits(points) == b"".join(struct.pack("<ddd", *r[:3]) for r in rows)
    assert bits(colors) == b"".join(struct.pack("<ddd", *(c / 255.0 for c in r[3:])) for r in rows)
    assert U.read_point_cloud(path)[0].tobytes() == points.tobytes()  # by the extension
    # CloudCompare's float scalar field as the label, big-endian
    head = ("ply\nformat binary_big_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "property float scalar_label\nend_header\n")
    path = write(tmp_path / "cc.PLY", head.encode() + b"".join(struct.pack(">ffff", 1.0, 2.0, 3.0, l) for l in (4.0, 2.5, -1.0)))
    points, colors, labels = U.read_point_cloud_ply(path, want_labels=True)
    assert bits(points) == struct.pack("<ddd", 1.0, 2.0, 3.0) * 3 and not colors.any() and labels.tolist() == [4, 0, -1]
    assert U.read_point_cloud(path)[0].tobytes() == points.tobytes()  # .PLY: the case of the extension is ignored
    with pytest.raises(ValueError):
        U.read_point_cloud(str(tmp_path / "a.xyz"))


# ---- PCD layouts ----------------------------------------------------------------------------------------------------------
def test_pcd_layouts(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    n = 300
    for name, data, stride, offsets, types, kind in R.general_pcd_files(n):
        path = write(tmp_path / (name + ".pcd"), data)
        with open(path, "rb") as f:
            lay = U.read_pcd_layout(f)
            assert len(f.read()) == n * stride  # left at the first payload byte
        assert (lay.stride, lay.n, lay.data) == (stride, n, "binary")
        assert lay.offsets == [int(x) for x in np.cumsum([0] + [s * c for s, c in zip(lay.sizes, lay.counts)])[:-1]]
        assert not U.pcd_is_words(lay) and U.pcd_slots(lay)[2] == kind
        got_o, got_t, _ = U.pcd_slots(lay)
        used = [k for k in range(7) if offsets[k] >= 0]
        assert [got_o[k] for k in used] == [offsets[k] for k in used] and [got_t[k] for k in used[:3]] == [types[k] for k in used[:3]]
        want_p, want_c, _, _ = R.unpack(data[-n * stride:], n, stride, offsets, types, kind)
        got_p, got_c = U.read_point_cloud_pcd(path)
        assert bits(got_p) == bits(want_p) and bits(got_c) == bits(want_c), name
    with open(write(tmp_path / "l.pcd", R.general_pcd_files(1)[1][1]), "rb") as f:
        lay = U.read_pcd_layout(f)
    assert (lay.fields, lay.sizes, lay.types, lay.counts) == ("x y z a _ b ring".split(), [4, 4, 4, 1, 1, 1, 2], list("FFFUUIU"), [1, 1, 1, 1, 3, 1, 1])
    assert lay.offsets == [0, 4, 8, 12, 13, 16, 17]
    for bad in (R.pcd_head("x y z".split(), [4, 4, 4], "FFF", [1] * 3, 1, "binary_compressed"),
                R.pcd_head("x y z".split(), [4, 4, 2], "FFF", [1] * 3, 1),    # F 2
                R.pcd_head("x y z".split(), [4, 4, 3], "FFU", [1] * 3, 1),    # SIZE 3
                R.pcd_head("x y z".split(), [4, 4, 4], "FFU", [1, 1, 0], 1)):  # COUNT 0
        with open(write(tmp_path / "bad.pcd", bad), "rb") as f:
            with pytest.raises(ValueError) as e:
                U.read_pcd_layout(f)
        if b"binary_compressed" in bad:
            assert "binary_compressed" in str(e.value)
    # a general ascii file: the tokens of every field, COUNT included
    head = R.pcd_head("x y z a _ rgb".split(), [8, 4, 4, 1, 2, 4], "FFFIUU", [1, 1, 1, 1, 2, 1], 2, "ascii")
    path = write(tmp_path / "a.pcd", head + b"0.1 2 -3.5 -7 1 2 16711935\n1e300 0 1 9 3 4 66051\n")
    p, c = U.read_point_cloud_pcd(path)
    assert bits(p) == struct.pack("<dddddd", 0.1, 2.0, -3.5, 1e300, 0.0, 1.0)
    assert bits(c) == struct.pack("<dddddd", 1.0, 0.0, 1.0, 1 / 255.0, 2 / 255.0, 3 / 255.0)


def test_word_pcd_files_read_as_before(pn2, tmp_path):
    """the 4-byte files tests/scene_io_ref.py makes: the same arrays as the model of the unchanged reader, binary and ascii"""
    U = pn2.util.point_cloud_util
    rs = np.random.RandomState(5)
    for fields in (["x", "y", "z", "rgb"], ["rgb", "x", "y", "z"], ["x", "y", "z", "intensity", "rgb"], ["x", "y", "z"]):
        rows = rs.randint(0, 2 ** 32, (50, len(fields)), dtype=np.uint64).astype(np.uint32)
        path = write(tmp_path / "w.pcd", S.pcd_bytes(fields, rows))
        with open(path, "rb") as f:
            lay = U.read_pcd_layout(f)
        assert U.pcd_is_words(lay) and lay.stride == 4 * len(fields) and lay.n == 50
        want_p, want_c = S.unpack_rows(rows, fields)
        got_p, got_c = U.read_point_cloud_pcd(path)
        assert bits(got_p) == bits(want_p) and bits(got_c) == bits(want_c)
    pts = rs.uniform(-9, 9, (20, 3))
    path = str(tmp_path / "asc.pcd")
    U.write_point_cloud_pcd(path, pts, rs.uniform(0, 1, (20, 3)), binary=False)
    with open(path, "rb") as f:
        assert U.read_pcd_layout(f).data == "ascii"
    assert bits(U.read_point_cloud_pcd(path)[0]) == bits(pts.astype(np.float32).astype(np.float64))


# ---- host writer and reader -------------------------------------------------------------------------------------------------
def test_host_writer_is_the_model_and_reads_back(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    n = 1100
    p64, p32, c64, u8, labels = R.ply_inputs(n)
    path = str(tmp_path / "w.ply")
    for coord, has_c, has_l in R.PACK_LAYOUTS:
        for points in (p64, p32):
            for colors in ((c64, u8) if has_c else (None,)):
                U.write_point_cloud_ply(path, points, colors, labels if has_l else None, coord)
                with open(path, "rb") as f:
                    data = f.read()
                payload = R.pack(points, colors, labels if has_l else None, coord)
                assert data == U.ply_header(n, coord, has_c, has_l).encode() + payload
                with open(path, "rb") as f:
                    offsets, types, kind = U.read_ply_header(f).slots
                want = R.unpack(payload, n, R.pack_stride(coord, has_c, has_l), offsets, types, kind, want_labels=has_l)
                got = U.read_point_cloud_ply(path, want_labels=has_l)
                assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
                if has_l:
                    assert got[2].dtype == np.int32 and np.array_equal(got[2], labels)
                with np.errstate(over="ignore"):
                    assert bits(got[0]) == bits(points.astype(np.float32).astype(np.float64) if coord == "float" else points.astype(np.float64))
    U.write_point_cloud_ply(path, p64[:0], c64[:0], labels[:0], "double")
    with open(path, "rb") as f:
        assert f.read() == U.ply_header(0, "double", True, True).encode()
    p, c, l = U.read_point_cloud_ply(path, want_labels=True)
    assert p.shape == (0, 3) and c.shape == (0, 3) and l.shape == (0,)


def test_host_reader_big_endian_and_ascii(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    n = 300
    for stride, offsets, types, kind in R.stride_cases()[:9]:
        names = {o: "x y z red green blue label".split()[k] for k, o in enumerate(offsets) if o >= 0}
        if kind == R.PACKED:
            continue  # PLY has no packed colour word
        # the layout as a PLY: filler properties of one byte between the fields
        props, at = [], 0
        spell = ["uchar", "char", "ushort", "short", "uint", "int", "float", "double"]
        by_off = {o: k for k, o in enumerate(offsets) if o >= 0}
        while at < stride:
            if at in by_off:
                props.append("property %s %s" % (spell[types[by_off[at]]], names[at]))
                at += R.SIZES[types[by_off[at]]]
            else:
                props.append("property uchar pad%d" % at)
                at += 1
        for big in (False, True):
            head = "ply\nformat binary_%s_endian 1.0\nelement vertex %d\n%s\nend_header\n" % (("little", "big")[big], n, "\n".join(props))
            rows = R.case_rows(n, stride, offsets, types, big, seed=stride)
            path = write(tmp_path / "e.ply", head.encode() + rows)
            has_l = offsets[6] >= 0
            want = R.unpack(rows, n, stride, offsets, types, kind, big, want_labels=has_l)
            got = U.read_point_cloud_ply(path, want_labels=has_l)
            assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]), (stride, big)
            if has_l:
                assert bits(got[2]) == bits(want[2])
    text = ("ply\nformat ascii 1.0\nelement vertex 3\nproperty double x\nproperty float y\nproperty short z\nproperty uchar red\n"
            "property ushort green\nproperty float blue\nproperty float label\nend_header\n"
            "0.1 0.1 -7 255 65535 0.25 3\n1e-320 1e-45 32767 0 1 nan 2.5\n-inf 3.5 0 128 256 -1.5 -2147483648\n")
    p, c, l = U.read_point_cloud_ply(write(tmp_path / "a.ply", text.encode()), want_labels=True)
    f32 = lambda v: struct.unpack("<f", struct.pack("<f", v))[0]  # noqa: E731
    assert bits(p) == struct.pack("<9d", 0.1, f32(0.1), -7.0, 1e-320, f32(1e-45), 32767.0, float("-inf"), 3.5, 0.0)
    assert bits(c[:, :2]) == struct.pack("<6d", 1.0, 1.0, 0.0, 1 / 65535.0, 128 / 255.0, 256 / 65535.0)
    assert c[0, 2] == 0.25 and np.isnan(c[1, 2]) and c[2, 2] == -1.5 and l.tolist() == [3, 0, -2 ** 31]


def test_unit_to_byte_edges(pn2, tmp_path):
    """0, 1, one ulp below 1, NaN, -0.0 and 1.5 through the model and through both host writers"""
    U = pn2.util.point_cloud_util
    c = np.array([0.0, 1.0, 1.0 - 2.0 ** -53, np.nan, -0.0, 1.5])
    want = [0, 255, 254, 0, 0, 255]
    assert R.unit_to_byte(c).tolist() == want
    colors = np.stack([c, c[::-1], np.roll(c, 3)], axis=1)
    path = str(tmp_path / "c.ply")
    U.write_point_cloud_ply(path, np.zeros((len(c), 3)), colors)
    got = U.read_point_cloud_ply(path)[1]
    assert bits(got[:, 0]) == bits(np.array(want) / 255.0) and bits(got[:, 1]) == bits(np.array(want[::-1]) / 255.0)
    # the .pcd writer's rule is the same (its numpy model leaves a NaN undefined: only the device says 0 there)
    assert S.pack_rows(np.zeros((len(c), 3)), np.nan_to_num(colors, nan=0.0))[:, 3].tolist() == [
        (r << 16) | (g << 8) | b for r, g, b in zip(want, want[::-1], np.roll(want, 3).tolist())]


def test_host_model_is_the_test_model(pn2):
    """util.point_cloud_util.unpack_records against tests/record_ref.py on every stride case, both byte orders"""
    U = pn2.util.point_cloud_util
    assert (U.REC_U8, U.REC_I8, U.REC_U16, U.REC_I16, U.REC_U32, U.REC_I32, U.REC_F32, U.REC_F64) == tuple(range(8))
    n = 257
    for stride, offsets, types, kind in R.stride_cases():
        for big in (False, True):
            rows = R.case_rows(n, stride, offsets, types, big, seed=stride)
            has_l = offsets[6] >= 0
            want = R.unpack(rows, n, stride, offsets, types, kind, big, want_labels=has_l)
            got = U.unpack_records(rows, n, stride, offsets, types, kind, big, want_labels=has_l)
            assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]) and got[3] == want[3], (stride, big)
            assert (got[2] is None and want[2] is None) or bits(got[2]) == bits(want[2])


# ---- the binding and the C ABI's refusals --------------------------------------------------------------------------------------
def test_entry_points_are_bound_and_exported(pn2):
    i, p = ctypes.c_int, ctypes.c_void_p
    sig = pn2._lib.SIGNATURES
    assert sig["pn2_record_unpack"] == [p, i, i, p, p, i, i, p, p, p, p, p]
    assert sig["pn2_record_pack"] == [p, i, p, i, p, i, i, i, p, p]
    c = pn2._lib.ABI.constants
    U = pn2.util.point_cloud_util
    names = ("U8", "I8", "U16", "I16", "U32", "I32", "F32", "F64")
    assert [c["PN2_REC_" + k] for k in names] == list(range(8)) == [getattr(U, "REC_" + k) for k in names] == [getattr(R, k) for k in names]
    assert (c["PN2_REC_COLOUR_NONE"], c["PN2_REC_COLOUR_THREE"], c["PN2_REC_COLOUR_PACKED"]) == (0, 1, 2) == (
        U.COLOUR_NONE, U.COLOUR_THREE, U.COLOUR_PACKED)
    assert c["PN2_REC_MAX_STRIDE"] == 1024 and c["PN2_REC_MAX_BYTES"] == 2 ** 31 - 16 and c["PN2_REC_SLOTS"] == 7
    assert c["PN2_REC_BIG_ENDIAN"] == 1 and c["PN2_ABI_VERSION"] == 2
    for name in ("write_point_cloud_ply", "read_point_cloud_ply", "read_point_cloud"):
        assert getattr(pn2, name) is getattr(pn2.scene_io, name)


def test_record_entry_points_refuse_bad_arguments_without_a_gpu(pn2):
    L, nul = pn2._lib.lib, None
    EINVAL, ENULL, ERANGE, EUNSUP = -1, -2, -3, -4
    ints = pn2._lib.int_array
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    odd16, odd8, odd4 = ctypes.c_void_p(4104), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    offsets, types = ints([0, 4, 8, 12, 13, 14, 15]), ints([R.F32] * 3 + [R.U8] * 3 + [R.I32])
    # rows, n, stride, offsets, types, colour_kind, flags, points, colors, labels, invalid, stream
    ok = [fake, 64, 19, offsets, types, R.THREE, 0, fake, fake, fake, fake, nul]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[("rows", "n", "stride", "offsets", "types", "kind", "flags", "points", "colors", "labels", "invalid").index(k)] = v
        return L.pn2_record_unpack(*args)

    # range and flags, before the pointers: every pointer NULL as well
    nulls = dict(rows=nul, offsets=nul, types=nul, points=nul)
    for kw in (dict(n=0), dict(n=-1), dict(stride=0), dict(stride=-3), dict(kind=3), dict(kind=-1), dict(flags=4), dict(flags=-1)):
        assert call(**kw) == EINVAL and call(**kw, **nulls) == EINVAL, kw
    assert call(stride=1025) == EUNSUP and call(stride=1025, **nulls) == EUNSUP
    for k in ("rows", "offsets", "types", "points"):
        assert call(**{k: nul}) == ENULL, k
    assert call(n=(2 ** 31 - 16) // 19 + 1) == ERANGE
    assert call(n=(2 ** 31 - 16) // 19 + 1, rows=nul) == ENULL  # the pointers before the product
    # the layout: an unknown type code, a field past the stride, overlapping fields, a wanted field that is absent
    assert call(types=ints([R.F32, 8, R.F32, 0, 0, 0, R.I32])) == EINVAL
    assert call(types=ints([R.F32, -1, R.F32, 0, 0, 0, R.I32])) == EINVAL
    assert call(stride=18) == EINVAL                                      # the label ends at 19
    assert call(offsets=ints([0, 4, 8, 12, 13, 14, 16])) == EINVAL        # the label would end at 20
    assert call(offsets=ints([0, 3, 8, 12, 13, 14, 15])) == EINVAL        # y overlaps x
    assert call(offsets=ints([0, 4, 8, 12, 13, 14, 11])) == EINVAL        # the label overlaps z and the colours
    assert call(offsets=ints([0, 4, 8, 12, 12, 14, 15])) == EINVAL        # two channels on one byte
    assert call(offsets=ints([0, 4, -1, 12, 13, 14, 15])) == EINVAL       # no z
    assert call(offsets=ints([0, 4, 8, 12, 13, 14, -1])) == EINVAL        # labels wanted, no label field
    # ... but a slot whose output is not asked for is not looked at: the call gets as far as a later check
    assert call(offsets=ints([0, 4, 8, 12, 13, 14, 11]), labels=nul, types=ints([R.F32] * 3 + [R.I8, R.U8, R.U8, R.I32])) == EUNSUP
    float_label = ints([R.F32] * 3 + [R.U8] * 3 + [R.F32])
    assert call(offsets=ints([0, 4, 8, 0, 0, 0, 15]), colors=nul, types=float_label, invalid=nul) == ENULL
    assert call(offsets=ints([0, 4, 8, 0, 0, 0, 15]), kind=R.NONE, types=float_label, invalid=nul) == ENULL
    # colour channel types
    assert call(types=ints([R.F32] * 3 + [R.I8, R.U8, R.U8, R.I32])) == EUNSUP
    assert call(types=ints([R.F32] * 3 + [R.U32, R.U8, R.U8, R.I32]), stride=64, offsets=ints([0, 4, 8, 12, 16, 17, 20])) == EUNSUP
    assert call(kind=R.PACKED, types=ints([R.F32] * 3 + [R.U16, 0, 0, R.I32])) == EUNSUP
    # a float label needs the counter
    assert call(types=ints([R.F32] * 3 + [R.U8] * 3 + [R.F32]), invalid=nul) == ENULL
    assert call(invalid=nul, rows=odd16) == EINVAL  # an integer label does not
    # alignment: rows 16 bytes, points and colors 8, labels 4, invalid 8
    for kw in (dict(rows=odd16), dict(rows=odd8), dict(points=odd8), dict(colors=odd8), dict(labels=odd4), dict(invalid=odd8)):
        assert call(**kw) == EINVAL, kw

    # points, point_kind, colors, color_kind, labels, n, coord_type, flags, rows, stream
    ok = [fake, 1, fake, 1, fake, 64, R.F64, 0, fake, nul]

    def pack(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[("points", "point_kind", "colors", "color_kind", "labels", "n", "coord", "flags", "rows").index(k)] = v
        return L.pn2_record_pack(*args)

    for kw in (dict(n=0), dict(n=-1), dict(point_kind=2), dict(point_kind=-1), dict(color_kind=3), dict(color_kind=-1), dict(coord=R.I32),
               dict(coord=8), dict(flags=1), dict(flags=4)):
        assert pack(**kw) == EINVAL and pack(points=nul, rows=nul, **kw) == EINVAL, kw
    for k in ("points", "colors", "rows"):
        assert pack(**{k: nul}) == ENULL, k
    assert pack(n=(2 ** 31 - 16) // 31 + 1) == ERANGE
    assert pack(n=(2 ** 31 - 16) // 31 + 1, labels=nul, rows=odd16) == EINVAL  # 27-byte rows fit; then the alignment
    for kw in (dict(rows=odd16), dict(points=odd8), dict(colors=odd8), dict(labels=odd4), dict(point_kind=0, points=odd4)):
        assert pack(**kw) == EINVAL, kw
