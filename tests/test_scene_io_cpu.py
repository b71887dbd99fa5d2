"""CPU tests of the scene-file writers and readers (scene_io.py, csrc/pn2_scene_io.hip): the host model tests/scene_io_ref.py
against the existing host writers and reader, the binding, the exports and the C ABI's refusals -- none needs a GPU."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_io_ref as R  # noqa: E402


def test_model_text_is_the_host_writers(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    rs = np.random.RandomState(3)
    for k, labels in enumerate([np.zeros(0, np.int32), np.array(R.edge_values(), np.int64), rs.randint(0, 9, 1000).astype(np.uint8),
                                rs.randint(-2 ** 31, 2 ** 31, 1000).astype(np.int32)]):
        path = str(tmp_path / ("l%d.labels" % k))
        U.write_labels(path, labels)
        with open(path, "rb") as f:
            assert f.read() == R.format_rows(labels)
        if len(labels):
            assert np.array_equal(U.load_labels(path), labels.astype(np.int32))
    assert R.format_rows(np.array([[1, -2], [30, 0]])) == b"1 -2\n30 0\n"
    assert R.format_rows([R.INT32_MIN, R.INT32_MAX]) == b"-2147483648\n2147483647\n"


def test_model_pcd_is_the_host_writers_and_readers(pn2, tmp_path):
    U = pn2.util.point_cloud_util
    colors = R.color_list()
    n = len(colors)
    rs = np.random.RandomState(4)
    cols = np.stack([colors, colors[::-1], np.roll(colors, 7)], axis=1)
    pts64 = np.resize(R.point_list(), (n, 3)) * 1.0
    pts32 = rs.uniform(-300, 300, (n, 3)).astype(np.float32)
    u8 = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    path = str(tmp_path / "a.pcd")
    for points, c in ((pts64, cols), (pts32, cols), (pts64, None), (pts32, None), (pts64[:1], cols[:1]), (pts64[:0], None)):
        with np.errstate(over="ignore"):
            U.write_point_cloud_pcd(path, points, c)
        with open(path, "rb") as f:
            assert f.read() == R.pcd_file_bytes(points, c)
        rows = R.pack_rows(points, c)
        want_p, want_c = U.read_point_cloud_pcd(path)
        got_p, got_c = R.unpack_rows(rows, ["x", "y", "z"] + (["rgb"] if c is not None else []))
        assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()
    # a uint8 colour is the word of the float64 colour c / 255.0
    assert np.array_equal(R.pack_rows(pts32, u8), R.pack_rows(pts32, u8.astype(np.float64) / 255.0))
    # the clip, and the header helper the device writer shares
    assert R.pack_rows(np.zeros((1, 3)), np.array([[-0.25, 1.5, 5e-324]]))[0, 3] == 0x00FF00
    assert R.pcd_bytes(["x", "y", "z", "rgb"], np.zeros((0, 4), np.uint32)) == U.pcd_header(0, True).encode()
    # other field orders through the host reader
    for fields in (["rgb", "x", "y", "z"], ["x", "y", "z", "intensity", "rgb"], ["x", "y", "z"]):
        rows = rs.randint(0, 2 ** 32, (50, len(fields)), dtype=np.uint64).astype(np.uint32)
        with open(path, "wb") as f:
            f.write(R.pcd_bytes(fields, rows))
        want_p, want_c = U.read_point_cloud_pcd(path)
        got_p, got_c = R.unpack_rows(rows, fields)
        assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()


def test_entry_points_are_bound_and_exported(pn2):
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    S = pn2._lib.SIGNATURES
    assert S["pn2_text_format_workspace_bytes"] == [i, p]
    assert S["pn2_text_format_i32"] == [p, i, i, p, z, p, p, z, p]
    assert S["pn2_pcd_pack"] == [p, i, p, i, i, p, p]
    assert S["pn2_pcd_unpack"] == [p, i, i, i, i, i, i, p, p, p]
    c = pn2._lib.ABI.constants
    assert c["PN2_TEXT_I32_CHARS"] == 12 and c["PN2_TEXT_FORMAT_ROWS"] == 256
    assert (c["PN2_PCD_F32"], c["PN2_PCD_F64"]) == (0, 1)
    assert (c["PN2_PCD_COLOR_NONE"], c["PN2_PCD_COLOR_F64"], c["PN2_PCD_COLOR_U8"]) == (0, 1, 2)
    for name in ("format_ints", "write_labels", "write_point_cloud_pcd", "read_point_cloud_pcd"):
        assert getattr(pn2, name) is getattr(pn2.scene_io, name)
    assert pn2.load_labels is pn2.preprocess.load_labels


def test_entry_points_refuse_bad_arguments_without_a_gpu(pn2):
    L, nul = pn2._lib.lib, None
    EINVAL, ENULL, ERANGE = -1, -2, -3
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    odd = ctypes.c_void_p(4100)
    out = (ctypes.c_ulonglong * 1)(0)
    assert L.pn2_text_format_workspace_bytes(0, out) == EINVAL
    assert L.pn2_text_format_workspace_bytes(-3, out) == EINVAL
    assert L.pn2_text_format_workspace_bytes(64, nul) == ENULL
    assert L.pn2_text_format_workspace_bytes((1 << 30) // 12 + 1, out) == ERANGE

    ok = [fake, 64, 2, fake, 4096, fake, fake, 1 << 20, nul]
    for at, value in ((1, 0), (1, -1), (2, 0), (2, -1), (2, 9)):
        args = list(ok)
        args[at] = value
        assert L.pn2_text_format_i32(*args) == EINVAL, (at, value)
    for at in (0, 3, 5, 6):  # values, text, out_bytes, workspace
        args = list(ok)
        args[at] = nul
        assert L.pn2_text_format_i32(*args) == ENULL, at
    args = list(ok)
    args[1], args[2] = (1 << 30) // 96 + 1, 8  # rows * cols * 12 > PN2_TEXT_MAX_BYTES
    assert L.pn2_text_format_i32(*args) == ERANGE
    args = list(ok)
    args[3] = odd  # text is 16-byte aligned
    assert L.pn2_text_format_i32(*args) == EINVAL

    ok = [fake, 1, fake, 1, 64, fake, nul]  # float64 points, float64 colours
    for at, value in ((4, 0), (4, -1), (1, 2), (1, -1), (3, 3), (3, -1)):  # n; an unknown point kind; an unknown colour kind
        args = list(ok)
        args[at] = value
        assert L.pn2_pcd_pack(*args) == EINVAL, (at, value)
    for at in (0, 2, 5):  # points, colors (a colour kind is given), rows
        args = list(ok)
        args[at] = nul
        assert L.pn2_pcd_pack(*args) == ENULL, at
    args = list(ok)
    args[4] = (1 << 27) + 1
    assert L.pn2_pcd_pack(*args) == ERANGE
    args = list(ok)
    args[5] = odd
    assert L.pn2_pcd_pack(*args) == EINVAL

    ok = [fake, 64, 4, 0, 1, 2, 3, fake, fake, nul]
    for at, value in ((1, 0), (1, -1), (2, 2), (2, 65), (3, 4), (4, -1), (5, 7), (6, 4), (6, -2)):
        args = list(ok)
        args[at] = value
        assert L.pn2_pcd_unpack(*args) == EINVAL, (at, value)
    for at in (0, 7):  # rows, points (colors may be NULL: want_colors=False)
        args = list(ok)
        args[at] = nul
        assert L.pn2_pcd_unpack(*args) == ENULL, at
    args = list(ok)
    args[1] = (1 << 27) + 1
    assert L.pn2_pcd_unpack(*args) == ERANGE
    args = list(ok)
    args[0] = odd
    assert L.pn2_pcd_unpack(*args) == EINVAL
