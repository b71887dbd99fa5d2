"""The raw-scan parser on the device (csrc/pn2_text.hip, preprocess.py) against the host model tests/text_parse_ref.py, BITWISE
(tobytes() equality: -0.0 and NaN count).  The kernels' own outputs -- line index, values, the per-token fast / slow flags -- are
compared before the host fallback fills anything in, so the fallback cannot mask a broken fast path."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_parse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

S3D = [R.F64, R.F64, R.F64, R.TRUNC_I32, R.I32, R.I32, R.I32]


def upload(data, cuda):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(cuda)


def check_raw(pn2, cuda, data, kinds, starts=True):
    """both kernels on one chunk, nothing filled in by the host: line index, flags, values of the well-formed lines, status"""
    m = R.parse(data, kinds)
    f64, i32, flags, line_start, (first, nbad, slow) = pn2.preprocess.parse_chunk(upload(data, cuda), kinds)
    if starts:
        assert line_start.cpu().tolist() == R.line_starts(data)
    assert line_start.numel() == len(m.flags) + 1
    assert flags.cpu().numpy().tobytes() == m.flags.tobytes()
    ok = (m.flags & R.MALFORMED) == 0
    assert f64.cpu().numpy()[ok].tobytes() == m.raw_f64[ok].tobytes()
    assert i32.cpu().numpy()[ok].tobytes() == m.raw_i32[ok].tobytes()
    kernel_bad = np.flatnonzero(~ok)
    assert nbad == len(kernel_bad) and first == (int(kernel_bad[0]) if len(kernel_bad) else None)
    assert slow == m.slow_tokens
    return m


def check_full(pn2, cuda, data, kinds, **kw):
    """parse_text: every value, slow tokens included, and the statistics"""
    m = R.parse(data, kinds)
    assert not m.bad
    f64, i32, stats = pn2.parse_text(data, kinds, device=cuda, **kw)
    assert f64.dtype == torch.float64 and i32.dtype == torch.int32
    assert f64.cpu().numpy().tobytes() == m.f64.tobytes() and tuple(f64.shape) == m.f64.shape
    assert i32.cpu().numpy().tobytes() == m.i32.tobytes() and tuple(i32.shape) == m.i32.shape
    assert stats.lines == len(m.flags) and stats.slow_tokens == m.slow_tokens
    return f64, i32, stats


def filler(nbytes, seed, newline_at_end):
    """nbytes of lines of varying length (0 to 40 bytes)"""
    rs = np.random.RandomState(seed)
    out = b""
    while len(out) < nbytes:
        out += b"7" * rs.randint(0, 41) + b"\n"
    return out[:nbytes - 1] + (b"\n" if newline_at_end else b"7")


def test_indexer_at_the_tile_edges(pn2, cuda):
    """files of T-1, T, T+1, 2T and 2T+1 bytes, with and without a final newline; a newline as the last byte of a tile, as the
    first byte of the next, and both"""
    T = pn2._lib.ABI.constants["PN2_TEXT_TILE_BYTES"]
    for nbytes in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        for end in (True, False):
            data = filler(nbytes, nbytes, end)
            assert len(data) == nbytes
            text = upload(data, cuda)
            want = R.line_starts(data)
            assert pn2.preprocess.index_lines(text).cpu().tolist() == want
            assert pn2.preprocess.index_lines(text, line_cap=2).cpu().tolist() == want  # too little room: the call is repeated
    for at in ((T - 1,), (T,), (T - 1, T), (2 * T - 1, 2 * T)):
        raw = bytearray(b"5" * (2 * T + 9))
        for p in at:
            raw[p] = 10
        data = bytes(raw)
        assert pn2.preprocess.index_lines(upload(data, cuda)).cpu().tolist() == R.line_starts(data), at
    # the lines on both sides of a tile edge parse: a blank line where the two newlines meet is malformed
    m = check_raw(pn2, cuda, b"5" * (T - 1) + b"\n" + b"6 \n" + b"7" * 20, [R.SKIP])
    assert m.flags.tolist() == [0, 0, 0]
    m = check_raw(pn2, cuda, b"5" * (T - 1) + b"\n\n" + b"7" * 20, [R.SKIP])
    assert m.flags.tolist() == [0, R.MALFORMED, 0]


def test_empty_and_single_line(pn2, cuda):
    f64, i32, stats = pn2.parse_text(b"", S3D, device=cuda)
    assert tuple(f64.shape) == (0, 3) and tuple(i32.shape) == (0, 4) and stats == (0, 0, 0)
    check_full(pn2, cuda, b"1.5", [R.F64])           # one line without a newline
    check_full(pn2, cuda, b"1.5\n", [R.F64])
    check_raw(pn2, cuda, b"-7", [R.I32])
    check_raw(pn2, cuda, b"\n", [R.I32])              # one blank line: malformed
    with pytest.raises(ValueError, match="line 1 "):
        pn2.parse_text(b"\n", [R.I32], device=cuda)


@pytest.mark.parametrize("nlines", [1, 63, 64, 65, 255, 256, 257])
def test_line_counts_around_the_wave_and_workgroup(pn2, cuda, nlines):
    rs = np.random.RandomState(nlines)
    body = b"\n".join(b"%d %.2f" % (v, w) for v, w in zip(rs.randint(-10 ** 9, 10 ** 9, nlines), rs.uniform(-1, 1, nlines)))
    for data in (body, body + b"\n"):
        m = check_raw(pn2, cuda, data, [R.I32, R.F64])
        assert len(m.flags) == nlines and not m.flags.any()


def test_long_lines(pn2, cuda):
    """a line longer than a tile of the index, and one longer than the span a workgroup stages in LDS (24 KiB): the workgroup
    that holds it reads global memory, its neighbours' lines included, and the values are the same"""
    T = pn2._lib.ABI.constants["PN2_TEXT_TILE_BYTES"]
    short = b"1.25 -3\n" * 300
    for length in (T + 77, 30000, 70001):
        long_line = b"0" * (length // 2) + b"12.5" + b" " * (length - length // 2 - 12) + b"\t-42\r"
        data = short + long_line + b"\n" + short + b"2.5 9"
        m = check_raw(pn2, cuda, data, [R.F64, R.I32])
        assert not m.flags.any() and m.f64[300, 0] == 12.5 and m.i32[300, 0] == -42 and len(m.flags) == 602
    # several KB of digits: a valid but slow token, and a bad one of the same length
    data = b"1 2\n" + b"1." + b"3" * 5000 + b" 4\n" + b"7" * 5000 + b"x 4\n5 6\n"
    m = check_raw(pn2, cuda, data, [R.F64, R.I32])
    assert m.flags.tolist() == [0, 1, R.MALFORMED, 0]


GRAMMAR = [b".5", b"5.", b"+1", b"-0.0", b"000.001", b"1e3", b"1E-3", b"1e+22", b"1e23", b"-0", b"+.5e-3", b"1.e5", b"0e0", b"-0e-22",
           b"123456789012345", b"1234567890123456", b"12345678901234567", b"1234567890123456789", b"12345678901234567890",
           b"9007199254740992", b"9007199254740993", b"9007199254740991", b"9007199254740992e22", b"9007199254740992e-22",
           b"9007199254740993e22", b"90071992547409.92e24", b"9007199254740992e23", b"9007199254740992e-23",
           b"1.5" + b"0" * 40, b"2" + b"0" * 15, b"2" + b"0" * 25, b"0." + b"0" * 21 + b"1", b"0." + b"0" * 22 + b"1",
           b"0" * 50 + b"1.5", b"1e0000000000000000000000005", b"1e99999999999999999999", b"1e-99999999999999999999", b"0e999",
           b"nan", b"NaN", b"-nan", b"inf", b"-INF", b"+Infinity", b"iNfInItY",
           b"2147483647", b"-2147483647", b"2147483647.99", b"-2147483647.99", b"-1234.5", b"1234.999", b"-0.9"]


def test_grammar_values_and_fast_slow_flags(pn2, cuda):
    """every token of the list as F64 and as TRUNC_I32: the kernel's per-token flags equal the model's, its fast values equal the
    model's bits; then parse_text: the slow ones, filled by the host, equal float(token)"""
    data = b"\n".join(b"%s %s" % (t, t) for t in GRAMMAR) + b"\n"
    m = check_raw(pn2, cuda, data, [R.F64, R.SKIP])
    assert 15 <= np.count_nonzero(m.flags) <= len(GRAMMAR) - 25  # both kinds of token are present in numbers
    check_full(pn2, cuda, data, [R.F64, R.SKIP])
    check_full(pn2, cuda, data, [R.F64, R.F64])
    finite = b"\n".join(b"%s %s" % (t, t) for t in GRAMMAR if R.trunc_i32(float(t)) is not None)
    m = check_raw(pn2, cuda, finite, [R.TRUNC_I32, R.F64])
    assert set(m.flags.tolist()) == {0, 3}
    check_full(pn2, cuda, finite, [R.TRUNC_I32, R.F64])
    # bit k of the flags is COLUMN k, skipped columns included
    m = check_raw(pn2, cuda, b"x 1e23 7 1e23 1.5 y 1e-23\n", [R.SKIP, R.F64, R.I32, R.TRUNC_I32, R.F64, R.SKIP, R.F64])
    assert m.flags.tolist() == [0b1001010]
    with pytest.raises(ValueError, match="line 1 "):  # a slow intensity that does not fit int32: found by the host fallback
        pn2.parse_text(b"1e23\n", [R.TRUNC_I32], device=cuda)
    with pytest.raises(ValueError, match="line 2 "):
        pn2.parse_text(b"1\nnan\n3e9\n", [R.TRUNC_I32], device=cuda)


def test_whitespace(pn2, cuda):
    data = (b"1.5 2 3\n" b"1.5\t2\t3\n" b"  1.5   2 \t 3  \n" b"1.5 2 3\r\n" b"\t1.5 2 3 \r\n" b"\r1.5\r2\r3\n" b"1.5 2 3")
    m = check_raw(pn2, cuda, data, [R.F64, R.I32, R.TRUNC_I32])
    assert not m.flags.any() and (m.f64 == 1.5).all() and (m.i32 == [2, 3]).all() and len(m.flags) == 7
    check_full(pn2, cuda, data, [R.F64, R.I32, R.TRUNC_I32])


GOOD = b"1.5 2.5 3.5 -7 1 2 3"


@pytest.mark.parametrize("bad", [b"1.2.3 2.5 3.5 -7 1 2 3", b"abc 2.5 3.5 -7 1 2 3", b"1.5 --1 3.5 -7 1 2 3", b"1.5 2.5 1e -7 1 2 3", b"",
                                 b"  \t\r", b"1.5 2.5 3.5 -7 1 2", b"1.5 2.5 3.5 -7 1 2 3 4", b"1.5 2.5 3.5 -7 1 1.5 3",
                                 b"1.5 2.5 3.5 3e9 1 2 3", b"1.5 2.5 3.5 -7 1 2 99999999999"])
def test_malformed_lines_are_named(pn2, cuda, bad):
    for at in (0, 3, 299):
        lines = [GOOD] * 300
        lines[at] = bad
        data = b"\n".join(lines) + b"\n"
        m = check_raw(pn2, cuda, data, S3D, starts=False)
        assert m.bad == [at]
        with pytest.raises(ValueError, match="line %d " % (at + 1)):
            pn2.parse_text(data, S3D, device=cuda)
        with pytest.raises(ValueError, match="line %d " % (at + 1)):  # the number counts lines of the FILE, not of the chunk
            pn2.parse_text(data, S3D, device=cuda, chunk_bytes=256)
    lines = [GOOD] * 300
    lines[200] = lines[41] = lines[299] = bad
    with pytest.raises(ValueError, match="line 42 "):  # the first of several
        pn2.parse_text(b"\n".join(lines), S3D, device=cuda)


@pytest.mark.parametrize("colour", [b"256", b"-1", b"1.5"])
def test_colours_outside_a_byte_are_named(pn2, cuda, tmp_path, colour):
    lines = [GOOD] * 100
    lines[57] = b"1.5 2.5 3.5 -7 1 " + colour + b" 3"
    lines[80] = b"1.5 2.5 3.5 -7 " + colour + b" 2 3"
    path = tmp_path / "scene.txt"
    path.write_bytes(b"\n".join(lines) + b"\n")
    with pytest.raises(ValueError, match="line 58 "):
        pn2.read_semantic3d_txt(str(path), cuda)


def test_chunked_parse_gives_the_same_bits(pn2, cuda, tmp_path):
    rs = np.random.RandomState(5)
    lines = [b"%.3f %.3f %.3f %d %d %d %d" % (x, y, z, i, r, g, b) for (x, y, z), i, (r, g, b) in
             zip(rs.uniform(-300, 300, (300, 3)).tolist(), rs.randint(-2000, 2000, 300).tolist(), rs.randint(0, 256, (300, 3)).tolist())]
    lines[17] = b"12345678.12345678901 1e23 -0.0 123456789012345678e-10 0 0 0"  # three slow tokens: their line is read back per chunk
    for data in (b"\n".join(lines) + b"\n", b"\n".join(lines)):
        one = check_full(pn2, cuda, data, S3D)
        assert one[2].chunks == 1 and one[2].slow_tokens == 3
        path = tmp_path / "chunked.txt"
        path.write_bytes(data)
        for chunk_bytes in (64, 4096):
            for source in (data, str(path), upload(data, cuda), torch.frombuffer(bytearray(data), dtype=torch.uint8)):
                f64, i32, stats = pn2.parse_text(source, S3D, device=cuda, chunk_bytes=chunk_bytes)
                assert f64.cpu().numpy().tobytes() == one[0].cpu().numpy().tobytes()
                assert i32.cpu().numpy().tobytes() == one[1].cpu().numpy().tobytes()
                assert stats.lines == 300 and stats.slow_tokens == 3 and stats.chunks >= len(data) // chunk_bytes
        with pytest.raises(ValueError, match="longer than a chunk"):
            pn2.parse_text(data, S3D, device=cuda, chunk_bytes=20)
        with pytest.raises(ValueError, match="longer than a chunk"):
            pn2.parse_text(upload(data, cuda), S3D, device=cuda, chunk_bytes=20)


# ---- the Semantic3D format at a size where every workgroup shape occurs -----------------------------------------------------------
N_SCENE = 200000


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """2e5 generated lines `%.3f %.3f %.3f %d %d %d %d`, coordinates within +-300, intensities of both signs, 1 in 50 of them a
    non-integer such as -1234.5; labels 0..8.  Parsed ONCE by the host model; nothing below changes it."""
    rs = np.random.RandomState(2024)
    xyz = rs.uniform(-300, 300, (N_SCENE, 3)) * (rs.uniform(0, 1, (N_SCENE, 1)) ** 3)  # dense near the origin: voxels with many points
    inten = rs.randint(-2047, 2048, N_SCENE).tolist()
    rgb = rs.randint(0, 256, (N_SCENE, 3)).tolist()
    lines = []
    for k, ((x, y, z), i, (r, g, b)) in enumerate(zip(xyz.tolist(), inten, rgb)):
        it = b"%d" % i if k % 50 else b"%.1f" % (i + (0.5 if i >= 0 else -0.5))
        lines.append(b"%.3f %.3f %.3f %s %d %d %d\n" % (x, y, z, it, r, g, b))
    data = b"".join(lines)
    labels = rs.randint(0, 9, N_SCENE).astype(np.int32)
    raw_dir = tmp_path_factory.mktemp("semantic_raw")
    (raw_dir / "scene.txt").write_bytes(data)
    with open(raw_dir / "scene.labels", "w") as f:
        f.write("".join("%d\n" % v for v in labels.tolist()))
    model = R.parse(data, S3D)
    assert not model.bad and len(model.flags) == N_SCENE
    return dict(dir=str(raw_dir), data=data, labels=labels, model=model, intensity=inten)


def test_semantic3d_scene_is_bit_equal_with_no_slow_token(pn2, cuda, scene):
    m = scene["model"]
    assert m.slow_tokens == 0 and not m.flags.any()  # the host model, on the CPU: this input has no slow token
    assert m.i32[:, 0].tolist() == scene["intensity"]  # -1234.5 -> -1234: toward zero
    assert (m.i32[:, 0] < 0).any() and (m.i32[:, 0] > 0).any() and np.abs(m.f64).max() <= 300.0
    f64, i32, stats = pn2.parse_text(os.path.join(scene["dir"], "scene.txt"), S3D, device=cuda)
    assert stats.slow_tokens == 0 and stats.lines == N_SCENE and stats.chunks == 1
    assert f64.cpu().numpy().tobytes() == m.f64.tobytes()
    assert i32.cpu().numpy().tobytes() == m.i32.tobytes()
    # the kernels alone: flags all zero, the same bits
    rf, ri, flags, _, status = pn2.preprocess.parse_chunk(upload(scene["data"], cuda), S3D)
    assert status == (None, 0, 0) and not bool(flags.any())
    assert rf.cpu().numpy().tobytes() == m.f64.tobytes() and ri.cpu().numpy().tobytes() == m.i32.tobytes()
    # several chunks through the pinned buffers: the same bits
    f64c, i32c, stats = pn2.parse_text(os.path.join(scene["dir"], "scene.txt"), S3D, device=cuda, chunk_bytes=1 << 20)
    assert stats.chunks >= 8 and stats.lines == N_SCENE and torch.equal(f64c, f64) and torch.equal(i32c, i32)


def host_arrays(scene, as_pcd=True):
    m = scene["model"]
    points = m.f64.astype(np.float32).astype(np.float64) if as_pcd else m.f64
    return points, m.i32[:, 1:4].astype(np.float64) / 255.0, m.i32[:, 0]


def test_read_semantic3d_txt_feeds_down_sample_arrays(pn2, cuda, scene):
    path = os.path.join(scene["dir"], "scene.txt")
    for as_pcd in (True, False):
        points, colors, intensity = pn2.read_semantic3d_txt(path, cuda, as_pcd=as_pcd)
        hp, hc, hi = host_arrays(scene, as_pcd)
        assert points.dtype == colors.dtype == torch.float64 and intensity.dtype == torch.int32
        assert points.cpu().numpy().tobytes() == hp.tobytes() and colors.cpu().numpy().tobytes() == hc.tobytes()
        assert intensity.cpu().numpy().tobytes() == hi.tobytes()
    points, colors, _ = pn2.read_semantic3d_txt(path, cuda)
    labels = pn2.load_labels(os.path.join(scene["dir"], "scene.labels"), cuda)
    assert labels.dtype == torch.int32 and labels.cpu().numpy().tobytes() == scene["labels"].tobytes()
    got = pn2.downsample.down_sample_arrays(points, colors, labels, voxel_size=0.5)
    hp, hc, _ = host_arrays(scene)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    want = pn2.downsample.down_sample_arrays(t(hp), t(hc), t(scene["labels"]), voxel_size=0.5)
    assert 1000 < got[0].shape[0] < N_SCENE
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


def test_txt_to_pcd_round_trip(pn2, cuda, scene, tmp_path, capsys):
    """point_cloud_txt_to_pcd + read_point_cloud_pcd == write_point_cloud_pcd of the host-parsed arrays + read_point_cloud_pcd
    (the writer, not the input colours: it floors c * 255)"""
    U = pn2.util.point_cloud_util
    pcd = os.path.join(scene["dir"], "scene.pcd")
    assert not os.path.exists(pcd)
    pn2.point_cloud_txt_to_pcd(scene["dir"], "scene", cuda)
    hp, hc, _ = host_arrays(scene)
    U.write_point_cloud_pcd(str(tmp_path / "host.pcd"), hp, hc)
    with open(pcd, "rb") as a, open(tmp_path / "host.pcd", "rb") as b:
        assert a.read() == b.read()
    gp, gc = U.read_point_cloud_pcd(pcd)
    wp, wc = U.read_point_cloud_pcd(str(tmp_path / "host.pcd"))
    assert gp.tobytes() == wp.tobytes() and gc.tobytes() == wc.tobytes() and gp.tobytes() == hp.tobytes()
    stamp = os.stat(pcd).st_mtime_ns
    capsys.readouterr()
    pn2.point_cloud_txt_to_pcd(scene["dir"], "scene", cuda)  # skipped when it exists
    assert "exists, skipped" in capsys.readouterr().out and os.stat(pcd).st_mtime_ns == stamp


def test_load_labels_equals_the_host_reader(pn2, cuda, tmp_path):
    U = pn2.util.point_cloud_util
    rs = np.random.RandomState(3)
    for n, end in ((1, True), (257, True), (5000, False)):
        labels = rs.randint(0, 9, n)
        path = str(tmp_path / ("l%d.labels" % n))
        U.write_labels(path, labels)
        if not end:
            with open(path, "rb+") as f:
                f.truncate(os.path.getsize(path) - 1)
        want = U.load_labels(path)
        got = pn2.load_labels(path, cuda)
        assert got.dtype == torch.int32 and got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes() and len(want) == n
