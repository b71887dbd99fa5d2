"""Raw Semantic3D scans on the device: <scene>.txt (`x y z intensity r g b` per line) and <scene>.labels (one integer per line)
become device tensors that feed downsample.down_sample_arrays directly.

The reference's preprocess.py:40-46 rewrites every line in a Python loop (tokens[3] = str(int(float(tokens[3])))), hands the
result to Open3D's .pts reader and .pcd writer, and downsample.py reads that file back; util/point_cloud_util.load_labels is one
int(line) per point.  Here the text is uploaded in chunks and parsed by two kernels (csrc/pn2_text.hip: a line index, then one
line per lane).  Numbers follow include/pn2_abi.h's rule: a token the device can convert with one correctly rounded operation is
converted there, every other valid token ("slow": more than 2^53 of mantissa, a large exponent, nan / inf) is flagged, read back
and converted by Python's own float(), so every value equals float(token) / int(token).

    points, colors, intensity = read_semantic3d_txt(path, device)      # (n,3) f64, (n,3) f64 in [0,1], (n,) int32
    labels = load_labels(path, device)                                  # (n,) int32
    f64, i32, stats = parse_text(data, [F64, F64, F64, TRUNC_I32, I32, I32, I32], device=device)
"""
import collections
import os

import numpy as np
import torch

from ._lib import ABI, aligned as _aligned, int_array, launch, ptr, workspace

F64, I32, TRUNC_I32, SKIP = (ABI.constants["PN2_TEXT_" + k] for k in ("F64", "I32", "TRUNC_I32", "SKIP"))
MALFORMED = ABI.constants["PN2_TEXT_MALFORMED"]
MAX_CHUNK_BYTES = ABI.constants["PN2_TEXT_MAX_BYTES"]
SEMANTIC3D_KINDS = (F64, F64, F64, TRUNC_I32, I32, I32, I32)  # x y z intensity r g b

Stats = collections.namedtuple("Stats", "lines slow_tokens chunks")
_BLANKS = bytes.maketrans(b"\t\r", b"  ")


def iter_chunks(readinto, buffers, chunk_bytes):
    """Cut a byte stream into chunks of whole lines.  readinto(memoryview) -> bytes read (0 at the end); buffers: two writable
    uint8 arrays of at least chunk_bytes (numpy views of pinned memory in parse_text), filled in turn.  Yields (which buffer, n):
    buffers[which][:n] ends with the last '\\n' inside the window of chunk_bytes, what follows it is carried to the front of
    the other buffer; the last chunk ends where the stream ends.  The consumer may read a buffer until it asks for the chunk
    after the next one.  A window without a '\\n' that is not the end of the stream: ValueError (a line longer than a chunk)."""
    carry, which, eof, offset = None, 0, False, 0
    while True:
        buf = buffers[which]
        n = 0 if carry is None else len(carry)
        if n:
            buf[:n] = carry
        while n < chunk_bytes and not eof:
            got = readinto(memoryview(buf)[n:chunk_bytes])
            if got:
                n += got
            else:
                eof = True
        if n == 0:
            return
        cut = n if eof else _last_newline(buf, n) + 1
        if cut == 0 and readinto(memoryview(np.empty(1, np.uint8))) == 0:
            eof, cut = True, n  # the stream ends with this window: its last line needs no '\n'
        if cut == 0:
            raise ValueError("the line at byte %d is longer than a chunk of %d bytes" % (offset, chunk_bytes))
        yield which, cut
        offset += cut
        if cut == n:
            if eof:
                return
            carry = None
        else:
            carry = buf[cut:n]
        which ^= 1


def _last_newline(buf, n):
    """index of the last '\\n' in buf[:n], -1 when there is none; searched from the end in growing windows"""
    hi, step = n, 4096
    while hi > 0:
        lo = max(0, hi - step)
        at = np.flatnonzero(buf[lo:hi] == 10)
        if len(at):
            return lo + int(at[-1])
        hi, step = lo, step * 4
    return -1


def _device_chunks(text, chunk_bytes):
    """iter_chunks for text that already lies on the device: yields views of whole lines"""
    pos, total = 0, text.numel()
    while pos < total:
        end = min(pos + chunk_bytes, total)
        if end < total:
            hi, step, cut = end, 4096, -1
            while hi > pos and cut < 0:
                lo = max(pos, hi - step)
                at = torch.nonzero(text[lo:hi] == 10)
                if at.numel():
                    cut = lo + int(at[-1])
                hi, step = lo, step * 4
            if cut < 0:
                raise ValueError("the line at byte %d is longer than a chunk of %d bytes" % (pos, chunk_bytes))
            end = cut + 1
        yield text[pos:end]
        pos = end


def index_lines(text, line_cap=None):
    """text: uint8 device tensor (16-byte aligned, whole lines) -> line_start int32 (nlines + 1,): line i is
    text[line_start[i] : line_start[i + 1] - 1].  Synchronises (the number of lines sizes what follows)."""
    nbytes, dev = text.numel(), text.device
    ws = workspace("pn2_text_index_workspace_bytes", dev, nbytes)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    if line_cap is None:  # from the density of '\n' at the front of the chunk, with room to spare
        head = text[:65536]
        line_cap = int(int((head == 10).sum()) * (nbytes / head.numel()) * 1.25) + 1024
    while True:
        starts = torch.empty((line_cap,), dtype=torch.int32, device=dev)
        launch("pn2_text_index_lines", dev, ptr(text), nbytes, ptr(starts), line_cap, ptr(count), ptr(ws), ws.numel())
        nlines = int(count.item())
        if nlines + 1 <= line_cap:
            return starts[:nlines + 1]
        line_cap = nlines + 1


def parse_chunk(text, kinds):
    """One chunk through both kernels, nothing filled in by the host: -> f64 (n,nF), i32 (n,nI), flags (n,) uint8, line_start,
    (first malformed line or None, malformed lines, slow tokens).  A slow token's value is whatever the output held."""
    kinds = [int(k) for k in kinds]
    dev = text.device
    line_start = index_lines(text)
    n = line_start.numel() - 1
    nf = sum(k == F64 for k in kinds)
    ni = sum(k in (I32, TRUNC_I32) for k in kinds)
    f64 = torch.zeros((n, nf), dtype=torch.float64, device=dev)
    i32 = torch.zeros((n, ni), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    status = torch.empty((3,), dtype=torch.int32, device=dev)
    launch("pn2_text_parse", dev, ptr(text), text.numel(), ptr(line_start), n, int_array(kinds), len(kinds),
           ptr(f64) if nf else None, ptr(i32) if ni else None, ptr(flags), ptr(status))
    first, bad, slow = status.tolist()
    return f64, i32, flags, line_start, (first if bad else None, bad, slow)


def _fill_slow(text, kinds, line_start, flags, f64, i32):
    """The flagged tokens through Python's float(): their lines' bytes are gathered on the device, read back in one copy and the
    values scattered into f64 / i32.  flags: the slow bits of the well-formed lines (zero elsewhere).  -> the smallest line index
    whose slow TRUNC_I32 token is not finite or not below 2^31 in magnitude (such a line is malformed), or None."""
    lines = torch.nonzero(flags).flatten()
    lo = line_start[lines].long()
    length = line_start[lines + 1].long() - 1 - lo
    offs = torch.cumsum(length, 0) - length
    gather = torch.arange(int(length.sum()), device=text.device) + torch.repeat_interleave(lo - offs, length)
    blob = text[gather].cpu().numpy().tobytes()
    fcol = {c: j for j, c in enumerate(c for c, k in enumerate(kinds) if k == F64)}
    icol = {c: j for j, c in enumerate(c for c, k in enumerate(kinds) if k in (I32, TRUNC_I32))}
    frow, fat, fval, irow, iat, ival, bad = [], [], [], [], [], [], None
    for line, fl, o, ln in zip(lines.tolist(), flags[lines].tolist(), offs.tolist(), length.tolist()):
        toks = [t for t in blob[o:o + ln].translate(_BLANKS).split(b" ") if t]
        for c in range(len(kinds)):
            if not fl >> c & 1:
                continue
            v = float(toks[c])
            if c in fcol:
                frow.append(line)
                fat.append(fcol[c])
                fval.append(v)
            elif v != v or not (-2147483648.0 < v < 2147483648.0):
                bad = line if bad is None else min(bad, line)
            else:
                irow.append(line)
                iat.append(icol[c])
                ival.append(int(v))
    dev = text.device
    if frow:
        f64[torch.tensor(frow, device=dev), torch.tensor(fat, device=dev)] = torch.tensor(fval, dtype=torch.float64, device=dev)
    if irow:
        i32[torch.tensor(irow, device=dev), torch.tensor(iat, device=dev)] = torch.tensor(ival, dtype=torch.int32, device=dev)
    return bad


def parse_text(data, kinds, device="cuda", chunk_bytes=256 << 20):
    """data: bytes, a uint8 tensor (host or device) or the path of a file; kinds: one of F64 / I32 / TRUNC_I32 / SKIP per column.
    -> f64 (lines, nF) float64 and i32 (lines, nI) int32 device tensors (columns in file order), Stats(lines, slow_tokens, chunks).
    Host data is streamed in chunks of at most chunk_bytes through two pinned buffers and a copy stream, so chunk k + 1 uploads
    while chunk k is parsed.  A malformed line raises ValueError with its 1-based line number in the file (the first one)."""
    kinds = [int(k) for k in kinds]
    if not 1 <= len(kinds) <= ABI.constants["PN2_TEXT_MAX_COLS"] or any(k not in (F64, I32, TRUNC_I32, SKIP) for k in kinds):
        raise ValueError("kinds: 1 to %d of F64, I32, TRUNC_I32, SKIP" % ABI.constants["PN2_TEXT_MAX_COLS"])
    chunk_bytes = int(chunk_bytes)
    if not 1 <= chunk_bytes <= MAX_CHUNK_BYTES:
        raise ValueError("chunk_bytes must lie in [1, %d]" % MAX_CHUNK_BYTES)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("parse_text runs on the MI355X only: got device %s" % dev)
    nf = sum(k == F64 for k in kinds)
    ni = sum(k in (I32, TRUNC_I32) for k in kinds)
    fparts, iparts, lines, slow_total, chunks = [], [], 0, 0, 0

    def finish(text):
        nonlocal lines, slow_total, chunks
        f64, i32, flags, line_start, (first, _, slow) = parse_chunk(text, kinds)
        if slow:
            late = _fill_slow(text, kinds, line_start, torch.where(flags >= MALFORMED, torch.zeros_like(flags), flags), f64, i32)
            first = late if first is None else (first if late is None else min(first, late))
        if first is not None:
            raise ValueError("line %d is malformed: expected %d column(s) of kinds %s" % (lines + first + 1, len(kinds), kinds))
        fparts.append(f64)
        iparts.append(i32)
        lines, slow_total, chunks = lines + f64.shape[0], slow_total + slow, chunks + 1

    with torch.cuda.device(dev):
        if isinstance(data, torch.Tensor) and data.is_cuda:
            if data.dtype != torch.uint8 or data.dim() != 1:
                raise ValueError("a text tensor is one-dimensional uint8")
            for view in _device_chunks(data.to(dev).contiguous(), chunk_bytes):
                if view.data_ptr() % 16:
                    aligned = _aligned(view.numel(), dev)
                    aligned.copy_(view)
                    view = aligned
                finish(view)
        else:
            _parse_host(data, chunk_bytes, dev, finish)
    if not fparts:  # no text at all
        fparts, iparts = [torch.zeros((0, nf), dtype=torch.float64, device=dev)], [torch.zeros((0, ni), dtype=torch.int32, device=dev)]
    if len(fparts) > 1:
        fparts, iparts = [torch.cat(fparts)], [torch.cat(iparts)]
    return fparts[0], iparts[0], Stats(lines, slow_total, chunks)


def _parse_host(data, chunk_bytes, dev, finish):
    """the upload pipeline of parse_text: chunk k is indexed and parsed on the caller's stream (finish waits for its line count and
    its status) only after chunk k + 1 has been read into the other pinned buffer and its copy queued on the copy stream, so
    that copy runs beside chunk k's kernels"""
    if isinstance(data, (str, os.PathLike)):
        src = open(data, "rb", buffering=0)
        total = os.fstat(src.fileno()).st_size
    else:
        if isinstance(data, torch.Tensor):
            if data.dtype != torch.uint8 or data.dim() != 1:
                raise ValueError("a text tensor is one-dimensional uint8")
            data = data.contiguous().numpy()
        view = memoryview(data).cast("B")
        src, total = _MemoryReader(view), len(view)
    try:
        size = max(1, min(chunk_bytes, total + 1))  # + 1: a file that fits is one chunk, its end seen by the first fill
        copy_stream = None
        pinned = [torch.empty((size,), dtype=torch.uint8).pin_memory() for _ in range(2)]
        text = [_aligned(size, dev) for _ in range(2)]
        copy_stream = torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)
        copied = [torch.cuda.Event(), torch.cuda.Event()]   # the upload of the buffer has finished (its pinned half is free)
        parsed = [torch.cuda.Event(), torch.cuda.Event()]   # the kernels that read the device half have finished
        pending = None
        chunks = iter_chunks(src.readinto, [p.numpy() for p in pinned], size)
        k = 0
        while True:
            if k >= 2:
                copied[k % 2].synchronize()  # the host is about to overwrite this pinned buffer
            nxt = next(chunks, None)
            if nxt is not None:
                which, n = nxt
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(parsed[which])  # recorded two chunks ago (a fresh event: no wait)
                    text[which][:n].copy_(pinned[which][:n], non_blocking=True)
                    copied[which].record(copy_stream)
            if pending is not None:
                pw, pn_ = pending
                main.wait_event(copied[pw])
                finish(text[pw][:pn_])
                parsed[pw].record(main)
            if nxt is None:
                return
            pending = nxt
            k += 1
    finally:
        if copy_stream is not None:
            copy_stream.synchronize()  # also on an error: no copy may outlive the buffers it reads and writes
        if hasattr(src, "close"):
            src.close()


class _MemoryReader:
    def __init__(self, view):
        self.view, self.pos = view, 0

    def readinto(self, out):
        n = min(len(out), len(self.view) - self.pos)
        out[:n] = self.view[self.pos:self.pos + n]
        self.pos += n
        return n


def read_semantic3d_txt(path, device="cuda", as_pcd=True, chunk_bytes=256 << 20):
    """<scene>.txt -> points (n,3) float64, colors (n,3) float64 in [0,1], intensity (n,) int32 = int(float(token)) as
    preprocess.py:44 leaves it.  r g b are integers in [0, 255] (anything else: ValueError naming the line).  as_pcd: xyz
    rounded through float32, which is what the reference's .txt -> .pts -> .pcd -> read_point_cloud round trip leaves in memory
    (the .pcd stores float32 coordinates and 8-bit colours)."""
    f64, i32, _ = parse_text(path, SEMANTIC3D_KINDS, device=device, chunk_bytes=chunk_bytes)
    rgb = i32[:, 1:4]
    outside = ((rgb < 0) | (rgb > 255)).any(dim=1)
    if bool(outside.any()):
        raise ValueError("line %d is malformed: a colour outside [0, 255]" % (int(torch.nonzero(outside)[0]) + 1))
    points = f64.to(torch.float32).to(torch.float64) if as_pcd else f64
    # c / 255.0 from a table divided on the host: torch divides a device tensor by a Python scalar as a multiplication by its
    # reciprocal, which is not the correctly rounded quotient np.asarray(pcd.colors) holds
    byte_to_unit = (torch.arange(256, dtype=torch.float64) / 255.0).to(rgb.device)
    return points, byte_to_unit[rgb.long()], i32[:, 0].contiguous()


def load_labels(path, device="cuda", chunk_bytes=256 << 20):
    """<scene>.labels, one integer per line -> int32 device tensor (util.point_cloud_util.load_labels on the device)"""
    _, i32, _ = parse_text(path, [I32], device=device, chunk_bytes=chunk_bytes)
    return i32[:, 0].contiguous()


def point_cloud_txt_to_pcd(raw_dir, file_prefix, device="cuda"):
    """preprocess.py:23-55: <raw_dir>/<file_prefix>.txt -> .pcd (binary, float32 xyz + packed rgb), skipped when it exists"""
    txt_file = os.path.join(raw_dir, file_prefix + ".txt")
    pcd_file = os.path.join(raw_dir, file_prefix + ".pcd")
    if os.path.isfile(pcd_file):
        print("pcd {} exists, skipped".format(pcd_file))
        return
    print("[txt->pcd]")
    print("txt: {}".format(txt_file))
    print("pcd: {}".format(pcd_file))
    points, colors, _ = read_semantic3d_txt(txt_file, device, as_pcd=True)
    from . import scene_io  # it imports this module
    scene_io.write_point_cloud_pcd(pcd_file, points, colors)
