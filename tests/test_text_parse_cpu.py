"""CPU tests of the raw-scan parser (preprocess.py, csrc/pn2_text.hip): the host model of its number rule against Python's own
float(), the chunk cutter, and the C ABI's refusals -- none needs a GPU."""
import ctypes
import os
import random
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_parse_ref as R  # noqa: E402


def bits(v):
    return struct.pack("<d", v)


def spell(rnd, w_digits, e10):
    """a token whose mantissa digits are w_digits and whose (exponent - fraction digits) is e10, spelled one of several ways"""
    nfrac = rnd.randint(0, len(w_digits))
    ip, fp = w_digits[:len(w_digits) - nfrac], w_digits[len(w_digits) - nfrac:]
    ex = e10 + nfrac
    tok = rnd.choice(["", "", "-", "+"]) + rnd.choice(["", "0", "000"]) + ip
    if fp or rnd.random() < 0.2:
        tok += "." + fp
    if ex or rnd.random() < 0.2:
        tok += rnd.choice("eE") + (rnd.choice(["", "+"]) if ex >= 0 else "") + str(ex)
    return tok.encode()


def test_fast_path_equals_float_on_random_tokens():
    """>= 1e5 random tokens, mantissas of 1 to 17 digits, e10 in [-25, 25]: every token the model calls fast has float(token)'s
    bits, and the classification is exactly (w <= 2^53 and |e10| <= 22)"""
    rnd = random.Random(20240229)
    fast = slow = 0
    for _ in range(150000):
        nd = rnd.randint(1, 17)
        digits = "".join(rnd.choice("0123456789") for _ in range(nd))
        e10 = rnd.randint(-25, 25)
        tok = spell(rnd, digits, e10)
        cls, v = R.classify_float(tok)
        want_fast = int(digits) <= 2 ** 53 and abs(e10) <= 22
        assert (cls == R.FAST) == want_fast and cls != R.BAD, tok
        if cls == R.FAST:
            assert bits(v) == bits(float(tok)), tok
            fast += 1
        else:
            slow += 1
    assert fast >= 100000 and slow >= 5000, (fast, slow)


@pytest.mark.parametrize("e10", [22, -22, 23, -23])
@pytest.mark.parametrize("w", [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1])
def test_fast_slow_boundary(w, e10):
    tok = ("%de%d" % (w, e10)).encode()
    cls, v = R.classify_float(tok)
    if w <= 2 ** 53 and abs(e10) <= 22:
        assert cls == R.FAST and bits(v) == bits(float(tok))
    else:
        assert cls == R.SLOW and v is None
    # the same number spelled with fraction digits: e10 = exponent - fraction digits decides, not the exponent
    s = str(w)
    cls2, v2 = R.classify_float(("-" + s[:5] + "." + s[5:] + "e%d" % (e10 + len(s) - 5)).encode())
    assert cls2 == cls and (v2 is None or bits(v2) == bits(-v))


def test_model_grammar():
    C = R.classify_float
    for tok, want in [(b".5", 0.5), (b"5.", 5.0), (b"+1", 1.0), (b"000.001", 0.001), (b"1e3", 1000.0), (b"1E-3", 0.001),
                      (b"1e+22", 1e22), (b"1.e1", 10.0), (b"9007199254740992", 9007199254740992.0)]:
        assert C(tok) == (R.FAST, want), tok
    assert bits(C(b"-0.0")[1]) == bits(-0.0) and bits(C(b"-0")[1]) == bits(-0.0)
    for tok in [b"1e23", b"9007199254740993", b"12345678901234567890", b"1.5" + b"0" * 30, b"nan", b"-INF", b"+Infinity", b"0e999"]:
        assert C(tok) == (R.SLOW, None), tok
        float(tok)  # valid for Python
    for tok in [b"1.2.3", b"abc", b"--1", b"1e", b".", b"+", b"e5", b".e5", b"1e5.0", b"infinit", b"1_0", b"0x10", b""]:
        assert C(tok) == (R.BAD, None), tok
    assert R.parse_int(b"-2147483648") == -2 ** 31 and R.parse_int(b"2147483648") is None and R.parse_int(b"1.5") is None
    assert R.parse_int(b"+7") == 7 and R.parse_int(b"-") is None
    assert R.trunc_i32(-1234.5) == -1234 and R.trunc_i32(3e9) is None and R.trunc_i32(-2147483648.0) is None
    assert R.split_lines(b"") == [] and R.split_lines(b"a") == [b"a"] and R.split_lines(b"a\n") == [b"a"]
    assert R.split_lines(b"a\n\nb") == [b"a", b"", b"b"] and R.split_lines(b"\n") == [b""]
    assert R.tokens(b" 1\t2  3 \r") == [b"1", b"2", b"3"] and R.tokens(b" \t\r") == []
    fl, f, i = R.parse_line(b"1.5 1e23 -1234.5 7 x", [R.F64, R.F64, R.TRUNC_I32, R.I32, R.SKIP])
    assert (fl, f, i) == (2, [1.5, None], [-1234, 7])
    assert R.parse_line(b"1 2", [R.F64])[0] == R.MALFORMED and R.parse_line(b"", [R.F64])[0] == R.MALFORMED
    assert R.parse_line(b"3e9", [R.TRUNC_I32])[0] == R.MALFORMED and R.parse_line(b"256", [R.I32]) == (0, [], [256])


class ShortReads:
    """a stream that hands out at most `most` bytes per call"""

    def __init__(self, data, most):
        self.data, self.pos, self.most = data, 0, most

    def readinto(self, out):
        n = min(len(out), self.most, len(self.data) - self.pos)
        out[:n] = self.data[self.pos:self.pos + n]
        self.pos += n
        return n


def cut(pn2, data, chunk_bytes, most=1 << 30):
    bufs = [np.full(chunk_bytes, 0x55, np.uint8) for _ in range(2)]
    return [bytes(bufs[which][:n]) for which, n in pn2.preprocess.iter_chunks(ShortReads(data, most).readinto, bufs, chunk_bytes)]


def whole_line_windows(data, chunk_bytes):
    """the rule of the cutter, written down independently: a window of chunk_bytes ends at its last '\n'; a shorter window, or
    one that reaches the end of the stream without a '\n', is the end of the stream; otherwise a line is longer than a chunk"""
    out, pos = [], 0
    while pos < len(data):
        win = data[pos:pos + chunk_bytes]
        k = win.rfind(b"\n")
        if len(win) < chunk_bytes or (k < 0 and pos + chunk_bytes == len(data)):
            out.append(win)
            break
        if k < 0:
            return None
        out.append(win[:k + 1])
        pos += k + 1
    return out


def test_chunk_cutter_at_every_cut_position(pn2):
    """a small file cut with every window size, read in pieces of 1, 3 and any number of bytes: the chunks are the rule's, they
    concatenate to the file, each but the last ends with '\n', none is longer than the window; a window shorter than a line raises"""
    raised = 0
    for data in [b"12 34\n5\n\n678 9 10\nab\n", b"12 34\n5\n\n678 9 10\nab", b"\n", b"x", b"", b"abc\ndefgh"]:
        for chunk_bytes in range(1, len(data) + 3):
            want = whole_line_windows(data, chunk_bytes)
            for most in (1, 3, 1 << 30):
                if want is None:
                    with pytest.raises(ValueError, match="longer than a chunk"):
                        cut(pn2, data, chunk_bytes, most)
                    raised += 1
                    continue
                parts = cut(pn2, data, chunk_bytes, most)
                assert parts == want, (data, chunk_bytes, most)
                assert b"".join(parts) == data and all(0 < len(p) <= chunk_bytes for p in parts)
                assert all(p.endswith(b"\n") for p in parts[:-1])
    assert raised >= 30
    assert cut(pn2, b"a\nbc", 3) == [b"a\n", b"bc"] and cut(pn2, b"a\nbc", 4) == [b"a\n", b"bc"] and cut(pn2, b"a\nbc", 5) == [b"a\nbc"]


def test_entry_points_are_bound(pn2):
    for name in ("pn2_text_index_workspace_bytes", "pn2_text_index_lines", "pn2_text_parse"):
        assert name in pn2._lib.SIGNATURES, name
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert pn2._lib.SIGNATURES["pn2_text_index_lines"] == [p, i, p, i, p, p, z, p]
    assert pn2._lib.SIGNATURES["pn2_text_parse"] == [p, i, p, i, p, i, p, p, p, p, p]
    assert pn2._lib.SIGNATURES["pn2_text_index_workspace_bytes"] == [i, p]
    for name in ("parse_text", "read_semantic3d_txt", "load_labels", "point_cloud_txt_to_pcd"):
        assert getattr(pn2, name) is getattr(pn2.preprocess, name)


def test_tile_constant_is_in_the_header(pn2):
    c = pn2._lib.ABI.constants
    assert c["PN2_TEXT_TILE_BYTES"] > 0 and c["PN2_TEXT_TILE_BYTES"] % 1024 == 0  # 64 lanes x 16 bytes per wave
    assert c["PN2_TEXT_MAX_BYTES"] == 1 << 30 and c["PN2_TEXT_MALFORMED"] == 128 and c["PN2_TEXT_MAX_COLS"] == 8
    assert (c["PN2_TEXT_F64"], c["PN2_TEXT_I32"], c["PN2_TEXT_TRUNC_I32"], c["PN2_TEXT_SKIP"]) == (R.F64, R.I32, R.TRUNC_I32, R.SKIP)
    assert pn2.preprocess.MALFORMED == R.MALFORMED


def test_entry_points_refuse_bad_arguments_without_a_gpu(pn2):
    L, nul = pn2._lib.lib, None
    EINVAL, ENULL, ERANGE, EUNSUP = -1, -2, -3, -4
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    out = (ctypes.c_ulonglong * 1)(0)
    assert L.pn2_text_index_workspace_bytes(0, out) == EINVAL
    assert L.pn2_text_index_workspace_bytes(-5, out) == EINVAL
    assert L.pn2_text_index_workspace_bytes(64, nul) == ENULL
    assert L.pn2_text_index_workspace_bytes((1 << 30) + 1, out) == ERANGE
    assert L.pn2_text_index_lines(fake, 0, fake, 8, fake, fake, 1 << 20, nul) == EINVAL
    assert L.pn2_text_index_lines(fake, 64, fake, 0, fake, fake, 1 << 20, nul) == EINVAL
    for hole in range(4):
        args = [fake, 64, fake, 8, fake, fake, 1 << 20, nul]
        args[(0, 2, 4, 5)[hole]] = nul
        assert L.pn2_text_index_lines(*args) == ENULL, hole
    assert L.pn2_text_index_lines(fake, (1 << 30) + 1, fake, 8, fake, fake, 1 << 20, nul) == ERANGE
    assert L.pn2_text_index_lines(ctypes.c_void_p(4100), 64, fake, 8, fake, fake, 1 << 20, nul) == EINVAL  # 16-byte aligned text

    kinds = lambda *k: (ctypes.c_int * len(k))(*k)  # noqa: E731
    ok = [fake, 64, fake, 2, kinds(R.F64, R.I32), 2, fake, fake, fake, fake, nul]
    for at, value in ((1, 0), (3, 0), (3, -1), (5, 0), (5, 9)):
        args = list(ok)
        args[at] = value
        assert L.pn2_text_parse(*args) == EINVAL, (at, value)
    for at in (0, 2, 4, 6, 7, 8, 9):  # text, line_start, kinds, out_f64 (an F64 column), out_i32 (an I32 column), flags, status
        args = list(ok)
        args[at] = nul
        assert L.pn2_text_parse(*args) == ENULL, at
    args = list(ok)
    args[4], args[7] = kinds(R.F64, R.SKIP), nul  # no int column: out_i32 may be NULL ... and the next fault is reported
    args[1] = (1 << 30) + 1
    assert L.pn2_text_parse(*args) == ERANGE
    args = list(ok)
    args[4] = kinds(R.F64, 4)
    assert L.pn2_text_parse(*args) == EINVAL
    args = list(ok)
    args[4], args[5] = kinds(*([R.I32] * 7 + [R.F64])), 8  # column 7's slow bit would be the malformed bit
    assert L.pn2_text_parse(*args) == EUNSUP
    args[4] = kinds(*([R.I32] * 7 + [R.TRUNC_I32]))
    assert L.pn2_text_parse(*args) == EUNSUP
    args = list(ok)
    args[0] = ctypes.c_void_p(4104)
    assert L.pn2_text_parse(*args) == EINVAL
