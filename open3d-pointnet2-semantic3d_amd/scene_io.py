"""Scene files written and read on the device: <scene>.labels (one integer per line) and binary <scene>.pcd, the files around
the predict flow (predict.py -> interpolate.py in the reference).

util.point_cloud_util.write_labels is one "%d\\n" % l per point on a .tolist() of the whole array, its .pcd writer and reader
work on host arrays.  Here labels are formatted and .pcd rows packed / unpacked by csrc/pn2_scene_io.hip; the bytes stream between
the device and the file in chunks through two pinned buffers and a copy stream (the pipeline of preprocess._parse_host, for
writes run backwards), so the file work of one chunk runs beside the device work and the copy of the next.  Every file has the
bytes of the host writer's, every array the bits of the host reader's.

    text = format_ints(values)                                  # uint8 device tensor: "%d" tokens, ' ' between, '\\n' per row
    write_labels(path, labels)                                  # labels: device tensor or array of any integer dtype
    write_point_cloud_pcd(path, points, colors=None)            # points f32 / f64, colors f64 in [0,1] or uint8
    points, colors = read_point_cloud_pcd(path, device)         # (n,3) f64, (n,3) f64 (None with want_colors=False)

Binary .ply files, and .pcd files whose fields are not all 4 bytes wide, are rows of any byte stride with typed fields at any
byte offset: csrc/pn2_records.hip unpacks and packs them, the headers are read and written by util.point_cloud_util.

    write_point_cloud_ply(path, points, colors=None, labels=None, coord="float")
    points, colors[, labels] = read_point_cloud_ply(path, device, want_labels=False)
    points, colors = read_point_cloud(path, device)             # by the extension: .pcd or .ply
"""
import os

import numpy as np
import torch

from ._lib import ABI, int_array, launch, ptr, u64_array
from .preprocess import _aligned
from .util import point_cloud_util

I32_CHARS = ABI.constants["PN2_TEXT_I32_CHARS"]
MAX_COLS = ABI.constants["PN2_TEXT_MAX_COLS"]
MAX_TEXT_BYTES = ABI.constants["PN2_TEXT_MAX_BYTES"]
MAX_PCD_ROWS = ABI.constants["PN2_PCD_MAX_ROWS"]
MAX_PCD_FIELDS = ABI.constants["PN2_PCD_MAX_FIELDS"]
_POINT_KINDS = {torch.float32: ABI.constants["PN2_PCD_F32"], torch.float64: ABI.constants["PN2_PCD_F64"]}
_COLOR_NONE, _COLOR_F64, _COLOR_U8 = (ABI.constants["PN2_PCD_COLOR_" + k] for k in ("NONE", "F64", "U8"))
MAX_REC_STRIDE = ABI.constants["PN2_REC_MAX_STRIDE"]
MAX_REC_BYTES = ABI.constants["PN2_REC_MAX_BYTES"]
_REC_BIG_ENDIAN = ABI.constants["PN2_REC_BIG_ENDIAN"]
_COORD_TYPES = {"float": (ABI.constants["PN2_REC_F32"], 12), "double": (ABI.constants["PN2_REC_F64"], 24)}
DEFAULT_CHUNK_ROWS = 1 << 20  # 12 MiB of label text at its worst case, 16 MiB of .pcd rows: per chunk one copy and one file call


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("scene_io runs on the MI355X only: got device %s" % dev)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _where(x):
    """the device the work runs on: a device tensor's own, else the current one"""
    return x.device if torch.is_tensor(x) and x.is_cuda else _device("cuda")


def _rows_i32(values, lo, hi, dev):
    """rows [lo, hi) of an integer tensor or array -> contiguous int32 on dev; a value outside int32: ValueError"""
    part = values[lo:hi]
    if not torch.is_tensor(part):
        part = np.ascontiguousarray(part)
        if part.dtype.kind not in "iu":
            raise ValueError("integers expected, got %s" % part.dtype)
        if part.dtype.itemsize >= 4 and part.dtype != np.int32 and part.size:
            if int(part.min()) < -2 ** 31 or int(part.max()) > 2 ** 31 - 1:
                raise ValueError("a value does not fit int32")
        return torch.from_numpy(part.astype(np.int32, copy=False)).to(dev)
    if part.dtype.is_floating_point or part.dtype.is_complex or part.dtype == torch.bool:
        raise ValueError("integers expected, got %s" % part.dtype)
    part = part.to(dev)
    if part.dtype != torch.int32 and part.element_size() >= 4 and part.numel():
        lo_v, hi_v = torch.aminmax(part)
        if int(lo_v) < -2 ** 31 or int(hi_v) > 2 ** 31 - 1:
            raise ValueError("a value does not fit int32")
    return part.to(torch.int32).contiguous()


class _Formatter:
    """the buffers of pn2_text_format_i32 for chunks of at most `rows` rows of `ncols` columns"""

    def __init__(self, rows, ncols, dev):
        if not 1 <= ncols <= MAX_COLS:
            raise ValueError("1 to %d columns, got %d" % (MAX_COLS, ncols))
        if rows * ncols * I32_CHARS > MAX_TEXT_BYTES:
            raise ValueError("a chunk of %d rows of %d columns exceeds %d bytes of text" % (rows, ncols, MAX_TEXT_BYTES))
        self.rows, self.ncols, self.dev = rows, ncols, dev
        need = u64_array([0])
        launch("pn2_text_format_workspace_bytes", dev, rows, need, stream=False)
        self.ws = _aligned(int(need[0]), dev)
        self.out_bytes = torch.zeros((1,), dtype=torch.int64, device=dev)

    def __call__(self, values, text):
        """values (n <= rows, ncols) int32 on the device -> queued; text (the worst case fits it) and out_bytes are its outputs"""
        launch("pn2_text_format_i32", self.dev, ptr(values), values.shape[0], self.ncols, ptr(text), text.numel(),
               ptr(self.out_bytes), ptr(self.ws), self.ws.numel())


def format_ints(values):
    """values: (n,) or (n, ncols <= 8) integers, a device tensor or an array -> the whole text as a uint8 device tensor: per row
    the "%d" tokens separated by one space and a '\\n' -- what parse_text reads back with I32 columns.  For tests and small
    writes: the worst case of 12 bytes per token is allocated.  Synchronises (the length sizes the result)."""
    dev = _where(values)
    shape = tuple(values.shape)
    if len(shape) not in (1, 2):
        raise ValueError("values: (n,) or (n, ncols)")
    n, ncols = shape[0], (shape[1] if len(shape) == 2 else 1)
    if n == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        fmt = _Formatter(n, ncols, dev)  # more than one call's range: ValueError (write_labels formats in chunks)
        text = _aligned(n * ncols * I32_CHARS, dev)
        fmt(_rows_i32(values, 0, n, dev).reshape(n, ncols), text)
        return text[:int(fmt.out_bytes.item())]


def _stream_out(f, dev, nchunks, buf_bytes, produce):
    """The download pipeline of the writers: produce(k, out) queues the device work that fills the device buffer `out` (buf_bytes
    uint8, 256-byte aligned) with chunk k on the caller's stream and returns how many bytes it made (it may synchronise for
    that).  Chunk k is copied to one of two pinned buffers on a copy stream and written to f while chunk k + 1 is produced and
    copied.  On an error no copy outlives the buffers it reads and writes."""
    copy_stream = None
    try:
        pinned = [torch.empty((buf_bytes,), dtype=torch.uint8).pin_memory() for _ in range(min(2, nchunks))]
        staged = [_aligned(buf_bytes, dev) for _ in range(min(2, nchunks))]
        copy_stream = torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)
        copied = [torch.cuda.Event(), torch.cuda.Event()]  # the copy out of staged[b] into pinned[b] has finished
        pending = None
        for k in range(nchunks):
            b = k % 2
            # staged[b] and pinned[b] held chunk k - 2: its copy was waited for and its bytes written one iteration ago
            nbytes = produce(k, staged[b])
            made = torch.cuda.Event()
            made.record(main)
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(made)
                pinned[b][:nbytes].copy_(staged[b][:nbytes], non_blocking=True)
                copied[b].record(copy_stream)
            if pending is not None:
                pb, pbytes = pending
                copied[pb].synchronize()
                f.write(memoryview(pinned[pb].numpy())[:pbytes])
            pending = (b, nbytes)
        if pending is not None:
            pb, pbytes = pending
            copied[pb].synchronize()
            f.write(memoryview(pinned[pb].numpy())[:pbytes])
    finally:
        if copy_stream is not None:
            copy_stream.synchronize()


def write_labels(path, labels, chunk_rows=DEFAULT_CHUNK_ROWS):
    """labels: (n,) integers, a device tensor or an array of any integer dtype -> the file of
    util.point_cloud_util.write_labels, byte for byte.  chunk_rows labels are formatted per call into a device buffer that holds
    their worst case (12 bytes each), so no call is repeated; n = 0 gives an empty file."""
    if len(tuple(labels.shape)) != 1:
        raise ValueError("labels: (n,)")
    n, chunk_rows = int(labels.shape[0]), int(chunk_rows)
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    with open(path, "wb") as f:
        if n == 0:
            return
        dev = _where(labels)
        with torch.cuda.device(dev):
            rows = min(chunk_rows, n)
            fmt = _Formatter(rows, 1, dev)

            def produce(k, out):
                fmt(_rows_i32(labels, k * rows, (k + 1) * rows, dev).reshape(-1, 1), out)
                return int(fmt.out_bytes.item())

            _stream_out(f, dev, (n + rows - 1) // rows, rows * I32_CHARS, produce)


def _rows_on(x, lo, hi, dev, dtypes, what):
    """rows [lo, hi) of a tensor or array of one of `dtypes` -> contiguous on dev"""
    part = x[lo:hi]
    if not torch.is_tensor(part):
        part = torch.from_numpy(np.ascontiguousarray(part))
    if part.dtype not in dtypes:
        raise ValueError("%s: got %s" % (what, part.dtype))
    return part.to(dev).contiguous()


def write_point_cloud_pcd(path, points, colors=None, chunk_rows=DEFAULT_CHUNK_ROWS):
    """points (n,3) float32 / float64, colors (n,3) float64 in [0,1] or uint8 (or None): device tensors or arrays -> a binary
    PCD v0.7 with FIELDS x y z [rgb], the file of util.point_cloud_util.write_point_cloud_pcd byte for byte (a uint8 colour c
    gives the word a float64 colour c / 255.0 gives).  The rows are packed on the device, chunk_rows per call."""
    n, chunk_rows = int(points.shape[0]), int(chunk_rows)
    if tuple(points.shape) != (n, 3) or (colors is not None and tuple(colors.shape) != (n, 3)):
        raise ValueError("points and colors: (n, 3)")
    if not 0 < chunk_rows <= MAX_PCD_ROWS:
        raise ValueError("chunk_rows must lie in [1, %d]" % MAX_PCD_ROWS)
    with open(path, "wb") as f:
        f.write(point_cloud_util.pcd_header(n, colors is not None, binary=True).encode())
        if n == 0:
            return
        dev = _where(points)
        row_bytes = 16 if colors is not None else 12
        with torch.cuda.device(dev):
            rows = min(chunk_rows, n)

            def produce(k, out):
                lo, hi = k * rows, (k + 1) * rows
                p = _rows_on(points, lo, hi, dev, _POINT_KINDS, "points: float32 or float64")
                c = None if colors is None else _rows_on(colors, lo, hi, dev, (torch.float64, torch.uint8),
                                                         "colors: float64 in [0, 1] or uint8")
                kind = _COLOR_NONE if c is None else (_COLOR_U8 if c.dtype == torch.uint8 else _COLOR_F64)
                launch("pn2_pcd_pack", dev, ptr(p), _POINT_KINDS[p.dtype], ptr(c), kind, p.shape[0], ptr(out))
                return p.shape[0] * row_bytes

            _stream_out(f, dev, (n + rows - 1) // rows, rows * row_bytes, produce)


def _stream_in(f, dev, total_bytes, chunk_bytes, consume, what="PCD"):
    """The upload pipeline of the reader (preprocess._parse_host for fixed-size chunks): the payload is read into two pinned
    buffers in turn, copied on a copy stream, and consume(k, device bytes) queues chunk k's kernels on the caller's stream
    while chunk k + 1 is read and copied.  A payload shorter than total_bytes: ValueError.  The device buffers end at a multiple
    of 16 bytes, so a kernel may read the 16-byte piece that a chunk's last byte lies in (pn2_record_unpack does)."""
    copy_stream = None
    try:
        nchunks = (total_bytes + chunk_bytes - 1) // chunk_bytes
        pinned = [torch.empty((chunk_bytes,), dtype=torch.uint8).pin_memory() for _ in range(min(2, nchunks))]
        staged = [_aligned((chunk_bytes + 15) & ~15, dev) for _ in range(min(2, nchunks))]
        copy_stream = torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)
        copied = [torch.cuda.Event(), torch.cuda.Event()]    # the upload of the buffer has finished (its pinned half is free)
        consumed = [torch.cuda.Event(), torch.cuda.Event()]  # the kernels that read the device half have finished
        for k in range(nchunks):
            b = k % 2
            nbytes = min(chunk_bytes, total_bytes - k * chunk_bytes)
            if k >= 2:
                copied[b].synchronize()  # the host is about to overwrite this pinned buffer
            view, got = memoryview(pinned[b].numpy())[:nbytes], 0
            while got < nbytes:
                step = f.readinto(view[got:])
                if not step:
                    raise ValueError("truncated %s payload: %d bytes missing" % (what, total_bytes - k * chunk_bytes - got))
                got += step
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(consumed[b])  # recorded two chunks ago (a fresh event: no wait)
                staged[b][:nbytes].copy_(pinned[b][:nbytes], non_blocking=True)
                copied[b].record(copy_stream)
            main.wait_event(copied[b])
            consume(k, staged[b][:nbytes])
            consumed[b].record(main)
    finally:
        if copy_stream is not None:
            copy_stream.synchronize()  # also on an error: no copy may outlive the buffers it reads and writes


def read_point_cloud_pcd(path, device="cuda", want_colors=True, chunk_rows=DEFAULT_CHUNK_ROWS):
    """-> points (n,3) float64, colors (n,3) float64 in [0,1] (zeros when the file has no rgb; None with want_colors=False) on
    the device, the bits of util.point_cloud_util.read_point_cloud_pcd.  The header is parsed on the host; a binary payload is
    streamed in chunks of chunk_rows whole rows and unpacked on the device; DATA ascii goes through the host reader.  Fields
    that are all 4 bytes with COUNT 1 are unpacked by pn2_pcd_unpack, any other layout (SIZE 1 / 2 / 8, COUNT above 1) by
    pn2_record_unpack; a row of more than PN2_REC_MAX_STRIDE bytes: ValueError."""
    dev = _device(device)
    chunk_rows = int(chunk_rows)
    if not 0 < chunk_rows <= MAX_PCD_ROWS:
        raise ValueError("chunk_rows must lie in [1, %d]" % MAX_PCD_ROWS)
    with open(path, "rb") as f:
        layout = point_cloud_util.read_pcd_layout(f)
        fields, n, data = layout.fields, layout.n, layout.data
        if data == "ascii":
            points, colors = point_cloud_util.read_point_cloud_pcd(path)
            return torch.from_numpy(points).to(dev), (torch.from_numpy(colors).to(dev) if want_colors else None)
        if not point_cloud_util.pcd_is_words(layout):
            return _unpack_stream(f, dev, n, layout.stride, point_cloud_util.pcd_slots(layout), False, want_colors, False,
                                  chunk_rows, "PCD")[:2]
        nf = len(fields)
        if nf > MAX_PCD_FIELDS:
            raise ValueError("a PCD row of more than %d fields" % MAX_PCD_FIELDS)
        ix, iy, iz = (fields.index(a) for a in "xyz")
        irgb = fields.index("rgb") if "rgb" in fields else -1
        with torch.cuda.device(dev):
            points = torch.empty((n, 3), dtype=torch.float64, device=dev)
            colors = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_colors else None
            if n:
                rows = min(chunk_rows, n)

                def consume(k, rows_bytes):
                    lo, m = k * rows, rows_bytes.numel() // (4 * nf)
                    launch("pn2_pcd_unpack", dev, ptr(rows_bytes), m, nf, ix, iy, iz, irgb, ptr(points[lo:lo + m]),
                           None if colors is None else ptr(colors[lo:lo + m]))

                _stream_in(f, dev, n * 4 * nf, rows * 4 * nf, consume)
        return points, colors


def _unpack_stream(f, dev, n, stride, slots, big, want_colors, want_labels, chunk_rows, what):
    """the payload of n records at f, streamed in chunks of whole rows through pn2_record_unpack -> points, colors, labels
    (None where not wanted).  slots: (offsets, types, colour kind) as util.point_cloud_util.unpack_records takes them."""
    offsets, types, colour_kind = slots
    if stride > MAX_REC_STRIDE:
        raise ValueError("a %s row of %d bytes: more than %d" % (what, stride, MAX_REC_STRIDE))
    with torch.cuda.device(dev):
        points = torch.empty((n, 3), dtype=torch.float64, device=dev)
        colors = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_colors else None
        labels = torch.empty((n,), dtype=torch.int32, device=dev) if want_labels else None
        invalid = torch.zeros((1,), dtype=torch.int64, device=dev)  # float labels that are no int32: they read as 0
        if n:
            rows = min(chunk_rows, n, MAX_REC_BYTES // stride)
            off_a, type_a = int_array(offsets), int_array(types)  # host arrays, read by the call

            def consume(k, rows_bytes):
                lo, m = k * rows, rows_bytes.numel() // stride
                launch("pn2_record_unpack", dev, ptr(rows_bytes), m, stride, off_a, type_a, colour_kind,
                       _REC_BIG_ENDIAN if big else 0, ptr(points[lo:lo + m]), None if colors is None else ptr(colors[lo:lo + m]),
                       None if labels is None else ptr(labels[lo:lo + m]), ptr(invalid))

            _stream_in(f, dev, n * stride, rows * stride, consume, what)
    return points, colors, labels


def read_point_cloud_ply(path, device="cuda", want_colors=True, want_labels=False, label_property=None,
                         chunk_rows=DEFAULT_CHUNK_ROWS):
    """-> points (n,3) float64, colors (n,3) float64 (zeros without red green blue; None with want_colors=False) [, labels (n,)
    int32 with want_labels] on the device, the bits of util.point_cloud_util.read_point_cloud_ply.  The header is parsed on the
    host; a binary payload of either byte order is streamed in chunks of chunk_rows whole rows and unpacked by
    pn2_record_unpack; format ascii goes through the host reader.  The label is the first present of label, class,
    scalar_label, or label_property; a float label that is no int32 reads as 0."""
    dev = _device(device)
    chunk_rows = int(chunk_rows)
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    with open(path, "rb") as f:
        h = point_cloud_util.read_ply_header(f, label_property)
        if want_labels and h.slots[0][6] < 0:
            raise ValueError("a PLY without a label property (one of %s)" % ", ".join(point_cloud_util.PLY_LABEL_NAMES))
        if h.format == "ascii":
            out = point_cloud_util.read_point_cloud_ply(path, want_labels, label_property)
            out = [torch.from_numpy(a).to(dev) for a in out]
            out[1] = out[1] if want_colors else None
        else:
            out = _unpack_stream(f, dev, h.n, h.stride, h.slots, h.format == "binary_big_endian", want_colors, want_labels,
                                 chunk_rows, "PLY")
    return tuple(out[:3]) if want_labels else tuple(out[:2])


def write_point_cloud_ply(path, points, colors=None, labels=None, coord="float", chunk_rows=DEFAULT_CHUNK_ROWS):
    """points (n,3) float32 / float64, colors (n,3) float64 in [0,1] or uint8, labels (n,) integers (or None): device tensors or
    arrays -> a binary little-endian PLY of x y z (coord: float or double) [red green blue uchar] [label int], the file of
    util.point_cloud_util.write_point_cloud_ply byte for byte.  The rows are packed on the device, chunk_rows per call; n = 0
    writes the header only."""
    n, chunk_rows = int(points.shape[0]), int(chunk_rows)
    if tuple(points.shape) != (n, 3) or (colors is not None and tuple(colors.shape) != (n, 3)) or (
            labels is not None and tuple(labels.shape) != (n,)):
        raise ValueError("points and colors: (n, 3), labels: (n,)")
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    header = point_cloud_util.ply_header(n, coord, colors is not None, labels is not None)  # coord is checked here
    coord_type, row_bytes = _COORD_TYPES[coord]
    row_bytes += (3 if colors is not None else 0) + (4 if labels is not None else 0)
    with open(path, "wb") as f:
        f.write(header.encode())
        if n == 0:
            return
        dev = _where(points)
        with torch.cuda.device(dev):
            rows = min(chunk_rows, n, MAX_REC_BYTES // row_bytes)

            def produce(k, out):
                lo, hi = k * rows, (k + 1) * rows
                p = _rows_on(points, lo, hi, dev, _POINT_KINDS, "points: float32 or float64")
                c = None if colors is None else _rows_on(colors, lo, hi, dev, (torch.float64, torch.uint8),
                                                         "colors: float64 in [0, 1] or uint8")
                lab = None if labels is None else _rows_i32(labels, lo, hi, dev)
                kind = _COLOR_NONE if c is None else (_COLOR_U8 if c.dtype == torch.uint8 else _COLOR_F64)
                launch("pn2_record_pack", dev, ptr(p), _POINT_KINDS[p.dtype], ptr(c), kind, ptr(lab), p.shape[0], coord_type, 0,
                       ptr(out))
                return p.shape[0] * row_bytes

            _stream_out(f, dev, (n + rows - 1) // rows, rows * row_bytes, produce)


def read_point_cloud(path, device="cuda", **kw):
    """read_point_cloud_pcd or read_point_cloud_ply by the extension of path (.pcd / .ply in either case), with their keywords;
    any other extension: ValueError"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".pcd":
        return read_point_cloud_pcd(path, device, **kw)
    if ext == ".ply":
        return read_point_cloud_ply(path, device, **kw)
    raise ValueError("a scene file is .pcd or .ply, got %s" % path)
