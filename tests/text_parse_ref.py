"""Pure-Python host model of the text parser's rule (include/pn2_abi.h "raw ASCII scans"), written from the rule and not from the
kernel: it splits lines, tokenises, classifies every token as fast / slow / bad with integer arithmetic and computes a fast
token's value with ONE float multiply or divide.  What the rule promises -- a fast value equals float(token) -- is checked against
Python's own float() in tests/test_text_parse_cpu.py; the device is compared with this model bit for bit."""
import re

import numpy as np

F64, I32, TRUNC_I32, SKIP = 0, 1, 2, 3
MALFORMED = 128
FAST, SLOW, BAD = 0, 1, 2
W_MAX = 2 ** 53
E10_MAX = 22
P10 = [float(10 ** k) for k in range(E10_MAX + 1)]  # exact in fp64 up to 10^22

_FLOAT = re.compile(rb"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?")
_SPECIAL = re.compile(rb"[+-]?(?:nan|inf|infinity)", re.I)
_INT = re.compile(rb"[+-]?[0-9]+")
_BLANKS = re.compile(rb"[ \t\r]+")


def split_lines(data):
    """a '\\n' ends a line; a last line without one is a line; nothing follows a final '\\n'"""
    if not data:
        return []
    lines = bytes(data).split(b"\n")
    if data[-1:] == b"\n":
        lines.pop()
    return lines


def line_starts(data):
    """the line index: entry i = first byte of line i, the last entry = one past the '\\n' that ends the last line (len + 1 when
    it has none), so line i is data[starts[i] : starts[i + 1] - 1]"""
    if not data:
        return []
    starts = [0] + [p + 1 for p in range(len(data) - 1) if data[p] == 10]
    return starts + [len(data) if data[-1] == 10 else len(data) + 1]


def tokens(line):
    return [t for t in _BLANKS.split(line) if t]


def mantissa(token):
    """-> (sign, w, e10) of a token of the decimal grammar, None otherwise.  A mantissa or an exponent of more than 20 significant
    digits is returned as 10^20 (with the exponent's sign): far outside the fast range either way, and Python refuses to convert
    digit strings of several thousand characters to int"""
    m = _FLOAT.fullmatch(token)
    if not m:
        return None
    sign, ip, fp, ex = m.groups()
    fp = fp or b""
    if not ip and not fp:
        return None
    digits = (ip + fp).lstrip(b"0") or b"0"
    w = int(digits) if len(digits) <= 20 else 10 ** 20
    e = 0
    if ex:
        edigits = ex.lstrip(b"+-").lstrip(b"0") or b"0"
        e = int(edigits) if len(edigits) <= 20 else 10 ** 20
        e = -e if ex[:1] == b"-" else e
    return sign, w, e - len(fp)


def classify_float(token):
    """-> (FAST, value) | (SLOW, None) | (BAD, None)"""
    parts = mantissa(token)
    if parts is None:
        return (SLOW, None) if _SPECIAL.fullmatch(token) else (BAD, None)
    sign, w, e10 = parts
    if w > W_MAX or abs(e10) > E10_MAX:
        return SLOW, None
    v = float(w) * P10[e10] if e10 >= 0 else float(w) / P10[-e10]
    return FAST, (-v if sign == b"-" else v)


def parse_int(token):
    """-> the int32 value of [+-]?digits+, None otherwise"""
    if not _INT.fullmatch(token):
        return None
    v = int(token)
    return v if -2 ** 31 <= v < 2 ** 31 else None


def trunc_i32(v):
    """int(v) toward zero when finite and |v| < 2^31, else None"""
    if v != v or not (-2147483648.0 < v < 2147483648.0):
        return None
    return int(v)


def parse_line(line, kinds):
    """-> (flags, f64 values, i32 values) as the device leaves them: a slow token's value is None (not written), and so is every
    value of a malformed line the model did not get to.  flags: bit k = column k is slow, MALFORMED = the line is bad."""
    toks = tokens(line)
    fvals = [None] * sum(k == F64 for k in kinds)
    ivals = [None] * sum(k in (I32, TRUNC_I32) for k in kinds)
    if len(toks) != len(kinds):
        return MALFORMED, fvals, ivals
    flags = nf = ni = 0
    for col, (tok, kind) in enumerate(zip(toks, kinds)):
        if kind == SKIP:
            continue
        if kind == I32:
            v = parse_int(tok)
            if v is None:
                flags |= MALFORMED
            ivals[ni] = v
            ni += 1
            continue
        cls, v = classify_float(tok)
        if cls == BAD:
            flags |= MALFORMED
        elif cls == SLOW:
            flags |= 1 << col
        if kind == F64:
            fvals[nf] = v
            nf += 1
        else:
            if cls == FAST:
                v = trunc_i32(v)
                if v is None:
                    flags |= MALFORMED
            ivals[ni] = v
            ni += 1
    return flags, fvals, ivals


class Parsed:
    """what parse() returns: flags (n,) uint8 as the device writes them; raw_f64 (n,nF) / raw_i32 (n,nI) as the kernel leaves
    zeroed outputs (a slow token's value not written; rows of malformed lines unspecified, zero here); f64 / i32 COMPLETE, the slow
    tokens filled with float(token) as the host fallback does; slow_tokens over the well-formed lines; bad = 0-based indices of
    the malformed lines, those found only by the fallback (a slow TRUNC_I32 token out of range) included"""


def parse(data, kinds):
    lines = split_lines(data)
    n = len(lines)
    out = Parsed()
    out.flags = np.zeros(n, np.uint8)
    out.f64 = np.zeros((n, sum(k == F64 for k in kinds)), np.float64)
    out.i32 = np.zeros((n, sum(k in (I32, TRUNC_I32) for k in kinds)), np.int32)
    out.raw_f64, out.raw_i32 = np.zeros_like(out.f64), np.zeros_like(out.i32)
    out.slow_tokens, out.bad = 0, []
    fcols = [c for c, k in enumerate(kinds) if k == F64]
    icols = [c for c, k in enumerate(kinds) if k in (I32, TRUNC_I32)]
    for i, line in enumerate(lines):
        flags, fvals, ivals = parse_line(line, kinds)
        out.flags[i] = flags
        if flags & MALFORMED:
            out.bad.append(i)
            continue
        if flags:
            out.raw_f64[i] = [0.0 if v is None else v for v in fvals]
            out.raw_i32[i] = [0 if v is None else v for v in ivals]
            toks = tokens(line)
            out.slow_tokens += bin(flags).count("1")
            for j, c in enumerate(fcols):
                if flags >> c & 1:
                    fvals[j] = float(toks[c])
            for j, c in enumerate(icols):
                if flags >> c & 1:
                    ivals[j] = trunc_i32(float(toks[c]))
            if any(v is None for v in ivals):
                out.bad.append(i)
                continue
        out.f64[i] = fvals
        out.i32[i] = ivals
        if not flags:
            out.raw_f64[i] = fvals
            out.raw_i32[i] = ivals
    return out
