"""The scene-file kernels and their Python callers on the device (csrc/pn2_scene_io.hip, scene_io.py) against the host model
tests/scene_io_ref.py and the host writers / reader of util/point_cloud_util.py.  Everything is compared as bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_io_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 256


def text_of(t):
    return t.cpu().numpy().tobytes()


def run_formatter(pn2, cuda, values, cap):
    """pn2_text_format_i32 into text = buffer[GUARD : GUARD + cap) of a poisoned buffer that is long enough for the whole text
    and a guard behind it -> the whole buffer as bytes, *out_bytes"""
    L, S = pn2._lib, pn2.scene_io
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32).reshape(len(values), -1)).to(cuda)
    nrows, ncols = v.shape
    room = nrows * ncols * 12 + GUARD
    buf = pn2.preprocess._aligned(GUARD + room, cuda)
    buf.fill_(POISON)
    need = L.u64_array([0])
    L.launch("pn2_text_format_workspace_bytes", cuda, nrows, need, stream=False)
    ws = pn2.preprocess._aligned(int(need[0]), cuda)
    out_bytes = torch.zeros((1,), dtype=torch.int64, device=cuda)
    L.launch("pn2_text_format_i32", cuda, L.ptr(v), nrows, ncols, L.ptr(buf, GUARD), cap, L.ptr(out_bytes), L.ptr(ws), ws.numel())
    assert S.I32_CHARS == 12
    return text_of(buf), int(out_bytes.item())


def check_contract(pn2, cuda, values, caps=None):
    """out_bytes == len(model); with text_cap = need, need - 1, need - 17 and 16 the prefix is the model's and every byte in
    front of text, at or past text_cap and past need is still poison"""
    want = R.format_rows(values)
    need = len(want)
    for cap in (caps or (need, need - 1, need - 17, 16)):
        if cap < 0:
            continue
        got, out_bytes = run_formatter(pn2, cuda, values, cap)
        assert out_bytes == need
        k = min(need, cap)
        assert got[:GUARD] == bytes([POISON]) * GUARD, cap
        assert got[GUARD:GUARD + k] == want[:k], cap
        assert got[GUARD + k:] == bytes([POISON]) * (len(got) - GUARD - k), cap


@pytest.mark.parametrize("ncols", [1, 2, 7, 8])
def test_formatter_values_in_every_column(pn2, cuda, ncols):
    """every edge value in every column position, beside neighbours of other widths"""
    edge = R.edge_values()
    rows = []
    for col in range(ncols):
        for k, v in enumerate(edge):
            row = [edge[(k + 3 * j + 1) % len(edge)] for j in range(ncols)]
            row[col] = v
            rows.append(row)
    values = np.array(rows, dtype=np.int64)
    assert values.min() == R.INT32_MIN and values.max() == R.INT32_MAX
    check_contract(pn2, cuda, values)
    assert text_of(pn2.format_ints(torch.from_numpy(values).to(cuda))) == R.format_rows(values)


def varying_rows(nrows, ncols, seed):
    """rows whose widths differ from row to row: every magnitude class, both signs"""
    rs = np.random.RandomState(seed)
    mag = 10 ** rs.randint(0, 10, (nrows, ncols)).astype(np.int64)
    v = np.minimum(rs.randint(0, 10, (nrows, ncols)) * mag // 3 + rs.randint(0, 2, (nrows, ncols)), R.INT32_MAX)
    return (v * rs.choice([-1, 1], (nrows, ncols))).astype(np.int32)


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_formatter_mapping_edges(pn2, cuda, nrows):
    for ncols in (1, 3):
        values = varying_rows(nrows, ncols, 100 * nrows + ncols)
        if nrows > 1:
            assert len({len(R.format_rows(values[i:i + 1])) for i in range(nrows)}) > 1
        check_contract(pn2, cuda, values)


def test_formatter_across_many_workgroups(pn2, cuda):
    """70 001 rows: more than 256 workgroups, the scan across tiles; 100 003 single-digit labels, the workload's own case"""
    values = varying_rows(70001, 2, 7)
    want = R.format_rows(values)
    check_contract(pn2, cuda, values, caps=(len(want), len(want) - 17))
    assert text_of(pn2.format_ints(torch.from_numpy(values).to(cuda))) == want
    labels = np.random.RandomState(8).randint(0, 9, 100003).astype(np.int32)
    want = R.format_rows(labels)
    assert len(want) == 2 * 100003
    check_contract(pn2, cuda, labels, caps=(len(want), len(want) - 1, 16))
    assert text_of(pn2.format_ints(torch.from_numpy(labels).to(cuda))) == want


@pytest.mark.parametrize("ncols", [1, 2, 7, 8])
def test_round_trip_through_the_parser(pn2, cuda, ncols):
    I32 = pn2.preprocess.I32
    edge = np.array(R.edge_values(), dtype=np.int64)
    values = np.concatenate([np.resize(edge, (len(edge) + 5, ncols)), varying_rows(1000, ncols, ncols)]).astype(np.int32)
    v = torch.from_numpy(values).to(cuda)
    text = pn2.format_ints(v)
    assert text.dtype == torch.uint8 and text.data_ptr() % 16 == 0
    f64, i32, flags, line_start, (first, bad, slow) = pn2.preprocess.parse_chunk(text, [I32] * ncols)
    assert first is None and bad == 0 and slow == 0 and not bool(flags.any())
    assert torch.equal(i32, v) and f64.shape == (len(values), 0)


def test_write_labels(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    rs = np.random.RandomState(11)
    want_path, got_path = str(tmp_path / "want.labels"), str(tmp_path / "got.labels")

    def same(labels, host, **kw):
        U.write_labels(want_path, host)
        pn2.write_labels(got_path, labels, **kw)
        with open(want_path, "rb") as a, open(got_path, "rb") as b:
            want, got = a.read(), b.read()
        assert got == want and want == R.format_rows(host)

    same(torch.zeros((0,), dtype=torch.int32, device=cuda), np.zeros(0, np.int32))  # an empty file
    same(torch.tensor([7], dtype=torch.int32, device=cuda), np.array([7]))
    labels = rs.randint(0, 9, 2501)
    for dtype in (torch.int64, torch.uint8, torch.int32):
        same(torch.from_numpy(labels).to(cuda, dtype), labels, chunk_rows=1000)  # three chunks: both pinned buffers reused
    same(labels, labels, chunk_rows=1000)                    # a numpy input (int64)
    same(labels.astype(np.uint8), labels, chunk_rows=2500)
    wide = np.concatenate([np.array(R.edge_values()), rs.randint(-2 ** 31, 2 ** 31, 3000)])
    same(torch.from_numpy(wide).to(cuda), wide, chunk_rows=999)
    same(torch.from_numpy(wide).to(cuda), wide)              # one chunk
    with pytest.raises(ValueError, match="int32"):
        pn2.write_labels(got_path, torch.tensor([2 ** 31], device=cuda))
    with pytest.raises(ValueError, match="int32"):
        pn2.write_labels(got_path, np.array([-2 ** 31 - 1]))


def pcd_inputs(n):
    colors = R.color_list()
    rs = np.random.RandomState(n)
    c64 = np.stack([np.resize(colors, n), np.resize(colors[::-1], n), np.resize(np.roll(colors, 341), n)], axis=1)
    if n >= len(colors):
        assert set(colors.tolist()) <= set(c64[:, 0].tolist())
    p64 = np.resize(R.point_list(), (n, 3)) * 1.0
    p32 = rs.uniform(-300, 300, (n, 3)).astype(np.float32)
    p32[::5] = np.resize(np.array([1e-45, -1e-40, 3.4e38, -0.0, np.inf], dtype=np.float32), (len(p32[::5]), 3))
    u8 = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    return p64, p32, c64, u8


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_pcd_pack_and_writer(pn2, cuda, tmp_path, n):
    U, L = pn2.util.point_cloud_util, pn2._lib
    p64, p32, c64, u8 = pcd_inputs(n)
    want_path, got_path = str(tmp_path / "want.pcd"), str(tmp_path / "got.pcd")
    t = lambda a: None if a is None else torch.from_numpy(a).to(cuda)  # noqa: E731
    kinds = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2}
    for points, colors in ((p64, c64), (p32, c64), (p64, u8), (p32, u8), (p64, None), (p32, None)):
        # the kernel's rows inside a poisoned buffer
        width = 3 if colors is None else 4
        buf = pn2.preprocess._aligned(GUARD + n * width * 4 + GUARD, cuda)
        buf.fill_(POISON)
        dp, dc = t(points), t(colors)
        L.launch("pn2_pcd_pack", cuda, L.ptr(dp), kinds[points.dtype], L.ptr(dc), 0 if colors is None else kinds[colors.dtype],
                 n, L.ptr(buf, GUARD))
        got = text_of(buf)
        assert got[GUARD:-GUARD] == R.pack_rows(points, colors).tobytes()
        assert got[:GUARD] == got[-GUARD:] == bytes([POISON]) * GUARD
        # the files: the host writer takes float64 colours, a uint8 colour c is c / 255.0 there
        host_colors = None if colors is None else (colors if colors.dtype == np.float64 else colors.astype(np.float64) / 255.0)
        with np.errstate(over="ignore"):
            U.write_point_cloud_pcd(want_path, points, host_colors)
        with open(want_path, "rb") as f:
            want = f.read()
        assert want == R.pcd_file_bytes(points, colors)
        for args, kw in (((dp, dc), {}), ((points, colors), {}), ((dp, dc), dict(chunk_rows=100))):
            pn2.write_point_cloud_pcd(got_path, *args, **kw)
            with open(got_path, "rb") as f:
                assert f.read() == want, (points.dtype, None if colors is None else colors.dtype, kw)


def test_pcd_writer_of_nothing(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    want_path, got_path = str(tmp_path / "want.pcd"), str(tmp_path / "got.pcd")
    U.write_point_cloud_pcd(want_path, np.zeros((0, 3)), np.zeros((0, 3)))
    pn2.write_point_cloud_pcd(got_path, torch.zeros((0, 3), dtype=torch.float64, device=cuda),
                              torch.zeros((0, 3), dtype=torch.float64, device=cuda))
    with open(want_path, "rb") as a, open(got_path, "rb") as b:
        assert a.read() == b.read()
    p, c = pn2.read_point_cloud_pcd(got_path, cuda)
    assert tuple(p.shape) == (0, 3) and tuple(c.shape) == (0, 3)


def as_bits(a):
    return a.cpu().numpy().view(np.int64) if torch.is_tensor(a) else np.ascontiguousarray(a).view(np.int64)


def reader_cases(n=777):
    rs = np.random.RandomState(21)
    words = lambda k: rs.randint(0, 2 ** 32, (n, k), dtype=np.uint64).astype(np.uint32)  # noqa: E731
    special = words(4)
    special[:6, :3] = np.array([np.nan, -0.0, np.inf, -np.inf, 1e-45, 0.0], dtype=np.float32).view(np.uint32)[:, None]
    special[:, 3] = np.resize(np.arange(256, dtype=np.uint32) * 0x010101, n)  # every byte value in every colour channel
    return [(["x", "y", "z", "rgb"], words(4)), (["x", "y", "z"], words(3)), (["rgb", "x", "y", "z"], words(4)),
            (["x", "y", "z", "intensity", "rgb"], words(5)), (["x", "y", "z", "rgb"], special)]


@pytest.mark.parametrize("case", range(5))
def test_pcd_unpack_and_reader(pn2, cuda, tmp_path, case):
    U = pn2.util.point_cloud_util
    fields, rows = reader_cases()[case]
    path = str(tmp_path / "in.pcd")
    with open(path, "wb") as f:
        f.write(R.pcd_bytes(fields, rows))
    want_p, want_c = U.read_point_cloud_pcd(path)
    model_p, model_c = R.unpack_rows(rows, fields)
    assert want_p.tobytes() == model_p.tobytes() and want_c.tobytes() == model_c.tobytes()
    for kw in ({}, dict(chunk_rows=300)):  # one upload, and three
        got_p, got_c = pn2.read_point_cloud_pcd(path, cuda, **kw)
        assert got_p.dtype == got_c.dtype == torch.float64 and got_p.is_cuda and got_c.is_cuda
        assert np.array_equal(as_bits(got_p), as_bits(want_p)) and np.array_equal(as_bits(got_c), as_bits(want_c)), kw
    got_p, none = pn2.read_point_cloud_pcd(path, cuda, want_colors=False, chunk_rows=300)
    assert none is None and np.array_equal(as_bits(got_p), as_bits(want_p))


def test_pcd_reader_of_host_written_and_ascii_files(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    p64, p32, c64, u8 = pcd_inputs(1025)
    path = str(tmp_path / "host.pcd")
    for points, colors, binary in ((p64, c64, True), (p32, None, True), (p32[:40], c64[:40], False), (p32[:40], None, False)):
        with np.errstate(over="ignore"):
            U.write_point_cloud_pcd(path, points, colors, binary=binary)
        want_p, want_c = U.read_point_cloud_pcd(path)
        got_p, got_c = pn2.read_point_cloud_pcd(path, cuda, chunk_rows=500)
        assert np.array_equal(as_bits(got_p), as_bits(want_p)) and np.array_equal(as_bits(got_c), as_bits(want_c))
        assert pn2.read_point_cloud_pcd(path, cuda, want_colors=False)[1] is None
    with open(path, "wb") as f:
        f.write(R.pcd_bytes(["x", "y", "z"], np.zeros((10, 3), np.uint32))[:-5])
    with pytest.raises(ValueError, match="truncated"):
        pn2.read_point_cloud_pcd(path, cuda)
