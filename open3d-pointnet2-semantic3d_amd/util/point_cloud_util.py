"""Label / point-cloud file helpers of the reference (util/point_cloud_util.py:53-63) plus a minimal PCD reader/writer
(the reference goes through Open3D's read_point_cloud / write_point_cloud, which is not available here)."""
import collections
import os
import struct

import numpy as np


def load_labels(label_path):
    """one int per line -> int32 array (point_cloud_util.py:53-57)"""
    with open(label_path, "r") as f:
        return np.array([int(line) for line in f], dtype=np.int32)


def write_labels(label_path, labels):
    """point_cloud_util.py:60-63"""
    with open(label_path, "w") as f:
        f.write("".join("%d\n" % l for l in np.asarray(labels).tolist()))


def pcd_header(n, has_colors, binary=True):
    """the header text of write_point_cloud_pcd (scene_io's device writer puts the same text in front of its payload)"""
    fields = "x y z rgb" if has_colors else "x y z"
    k = 4 if has_colors else 3
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\n"
            "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (
                fields, " ".join(["4"] * k), " ".join(["F"] * k), " ".join(["1"] * k), n, n, "binary" if binary else "ascii"))


def _pcd_meta(f):
    """the header lines of a .pcd opened "rb", key -> tokens; f is left at the first payload byte"""
    meta = {}
    while True:
        line = f.readline().decode("ascii", "replace").strip()
        if not line or line.startswith("#"):
            if not line:
                raise ValueError("truncated PCD header")
            continue
        key, _, val = line.partition(" ")
        meta[key] = val.split()
        if key == "DATA":
            return meta


def read_pcd_header(f):
    """f: a .pcd opened "rb" -> fields (names), number of points, "binary" / "ascii"; f is left at the first payload byte"""
    meta = _pcd_meta(f)
    fields, n = meta["FIELDS"], int(meta["POINTS"][0])
    sizes = [int(s) for s in meta["SIZE"]]
    if any(s != 4 for s in sizes) or any(t not in "FUI" for t in meta["TYPE"]):
        raise ValueError("only 4-byte PCD fields are supported")
    if meta["DATA"][0] not in ("binary", "ascii"):
        raise ValueError("unsupported PCD DATA %s" % meta["DATA"][0])
    return fields, n, meta["DATA"][0]


def write_point_cloud_pcd(path, points, colors=None, binary=True):
    """PCD v0.7 with FIELDS x y z [rgb] (float32; rgb packed 0x00RRGGBB in a float, as Open3D / PCL write it)."""
    points = np.asarray(points, dtype=np.float32)
    n = len(points)
    has_c = colors is not None
    header = pcd_header(n, has_c, binary)
    cols = [points]
    if has_c:
        c8 = np.clip(np.floor(np.asarray(colors, dtype=np.float64) * 255.0), 0, 255).astype(np.uint32)
        packed = ((c8[:, 0] << 16) | (c8[:, 1] << 8) | c8[:, 2]).astype(np.uint32).view(np.float32)
        cols.append(packed[:, None])
    data = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.float32)
    with open(path, "wb") as f:
        f.write(header.encode())
        if binary:
            f.write(data.tobytes())
        else:
            for row in data:
                f.write((" ".join(repr(float(v)) for v in row) + "\n").encode())


def read_point_cloud_pcd(path):
    """-> points (n,3) float64, colors (n,3) float64 in [0,1] (zeros when the file has no rgb), like np.asarray(pcd.points)
    / np.asarray(pcd.colors) after open3d.read_point_cloud.  A file whose fields are all 4 bytes with COUNT 1 is read as it
    always was (every word of x y z a float32); any other layout goes through read_pcd_layout and unpack_records."""
    with open(path, "rb") as f:
        layout = read_pcd_layout(f)
        if not pcd_is_words(layout):
            offsets, types, colour_kind = pcd_slots(layout)
            rec = _read_records(f, layout.n, layout.stride, _pcd_columns(layout), layout.data == "ascii", "PCD")
            return unpack_records(rec, layout.n, layout.stride, offsets, types, colour_kind)[:2]
        f.seek(0)
        fields, n, data = read_pcd_header(f)
        if data == "binary":
            raw = np.frombuffer(f.read(n * 4 * len(fields)), dtype=np.float32).reshape(n, len(fields))
        else:
            raw = np.array([[struct.unpack("f", struct.pack("f", float(v)))[0] for v in f.readline().split()]
                            for _ in range(n)], dtype=np.float32).reshape(n, len(fields))
    xyz = np.stack([raw[:, fields.index(a)] for a in "xyz"], axis=1).astype(np.float64)
    if "rgb" in fields:
        p = np.ascontiguousarray(raw[:, fields.index("rgb")]).view(np.uint32)
        colors = np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], axis=1).astype(np.float64) / 255.0
    else:
        colors = np.zeros_like(xyz)
    return xyz, colors


# ---- records: rows of any byte stride with typed fields at any byte offset -- the host model of csrc/pn2_records.hip -----------
# The type codes and colour kinds are include/pn2_abi.h's PN2_REC_* (tests/test_records_cpu.py holds the two together).
REC_U8, REC_I8, REC_U16, REC_I16, REC_U32, REC_I32, REC_F32, REC_F64 = range(8)
REC_SIZES = (1, 1, 2, 2, 4, 4, 4, 8)
REC_NUMPY = ("u1", "i1", "u2", "i2", "u4", "i4", "f4", "f8")
COLOUR_NONE, COLOUR_THREE, COLOUR_PACKED = range(3)
SLOTS = ("x", "y", "z", "c0", "c1", "c2", "label")
_CHANNEL_TYPES = (REC_U8, REC_U16, REC_F32, REC_F64)


def unpack_records(raw, n, stride, offsets, types, colour_kind, big=False, want_labels=False):
    """raw: n records of `stride` bytes; offsets / types: per slot of SLOTS the byte offset (-1: absent) and the REC_* code ->
    points (n,3) float64 (the values, exact), colors (n,3) float64, labels (n,) int32 (None unless wanted), invalid.
    The colour rules are this project's own: a U8 channel is byte / 255.0, a U16 channel v / 65535.0, a float channel the value
    itself; COLOUR_PACKED reads a 4-byte word 0x00RRGGBB at c0, each byte / 255.0; COLOUR_NONE gives zeros.  An integer label
    becomes int32 (U32 reinterpreted); a float label that is not finite, integral and inside int32 is 0 and counted in invalid."""
    end = ">" if big else "<"
    used = [k for k in range(7) if offsets[k] >= 0 and (k < 3 or (k < 6 and k - 3 < (0, 3, 1)[colour_kind]) or (k == 6 and want_labels))]
    if any(k not in used for k in (0, 1, 2)) or (want_labels and 6 not in used):
        raise ValueError("a record needs x, y and z, and a label field when labels are wanted")
    formats = [end + ("u4" if k == 3 and colour_kind == COLOUR_PACKED else REC_NUMPY[types[k]]) for k in used]
    rec = np.frombuffer(raw, dtype=np.dtype({"names": [SLOTS[k] for k in used], "formats": formats,
                                             "offsets": [offsets[k] for k in used], "itemsize": stride}), count=n)
    with np.errstate(invalid="ignore"):  # a signalling float32 NaN is quieted by the conversion
        points = np.stack([rec[a].astype(np.float64) for a in "xyz"], axis=1)
        if colour_kind == COLOUR_THREE:
            if any(types[k] not in _CHANNEL_TYPES for k in (3, 4, 5)):
                raise ValueError("a colour channel is uint8, uint16, float32 or float64")
            full = {REC_U8: 255.0, REC_U16: 65535.0}  # an integer channel is v / its largest value, a float channel itself
            channel = [rec[SLOTS[k]].astype(np.float64) for k in (3, 4, 5)]
            colors = np.stack([c / full[types[k]] if types[k] in full else c for k, c in zip((3, 4, 5), channel)], axis=1)
        elif colour_kind == COLOUR_PACKED:
            if REC_SIZES[types[3]] != 4:
                raise ValueError("a packed colour is one 4-byte word")
            w = rec["c0"].astype(np.uint32)
            colors = np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1).astype(np.float64) / 255.0
        else:
            colors = np.zeros_like(points)
        labels, invalid = None, 0
        if want_labels:
            v = rec["label"]
            if types[6] >= REC_F32:
                d = v.astype(np.float64)
                ok = np.isfinite(d) & (d == np.floor(d)) & (d >= -2.0 ** 31) & (d <= 2.0 ** 31 - 1)
                labels, invalid = np.where(ok, d, 0.0).astype(np.int32), int(n - ok.sum())
            else:
                labels = v.astype(np.uint32).view(np.int32) if types[6] == REC_U32 else v.astype(np.int32)
    return points, colors, labels, invalid


def _read_records(f, n, stride, columns, ascii, what):
    """the payload of n records as bytes.  binary: read as it lies; ascii: one line of tokens per record, parsed per column
    (numpy format, count, offset) into little-endian records of the same layout."""
    if not ascii:
        raw = f.read(n * stride)
        if len(raw) < n * stride:
            raise ValueError("truncated %s payload: %d bytes missing" % (what, n * stride - len(raw)))
        return raw
    names = ["f%d" % k for k in range(len(columns))]
    rec = np.zeros(n, np.dtype({"names": names, "formats": [("<" + fmt, (count,)) for fmt, count, _ in columns],
                                "offsets": [off for _, _, off in columns], "itemsize": stride}))
    rows = [f.readline().split() for _ in range(n)]
    ntokens = sum(count for _, count, _ in columns)
    if any(len(r) != ntokens for r in rows):
        raise ValueError("truncated %s payload: a line without its %d values" % (what, ntokens))
    at = 0
    for name, (fmt, count, _) in zip(names, columns):
        conv = float if fmt[0] == "f" else int
        with np.errstate(over="ignore"):
            rec[name] = np.array([[conv(t) for t in r[at:at + count]] for r in rows], dtype=fmt).reshape(n, count)
        at += count
    return rec.tobytes()


PcdLayout = collections.namedtuple("PcdLayout", "fields sizes types counts stride offsets n data")
_PCD_CODES = {("U", 1): REC_U8, ("I", 1): REC_I8, ("U", 2): REC_U16, ("I", 2): REC_I16, ("U", 4): REC_U32, ("I", 4): REC_I32,
              ("F", 4): REC_F32, ("F", 8): REC_F64}


def read_pcd_layout(f):
    """f: a .pcd opened "rb" -> PcdLayout: the field names, SIZE (1, 2, 4, 8), TYPE (I, U, F) and COUNT (>= 1) of each, the row
    stride, the byte offset of each field, the number of points and DATA ("binary" / "ascii"); f is left at the first payload
    byte.  DATA binary_compressed and an impossible pair such as F 2: ValueError."""
    meta = _pcd_meta(f)
    fields, types = meta["FIELDS"], meta["TYPE"]
    sizes = [int(s) for s in meta["SIZE"]]
    counts = [int(c) for c in meta["COUNT"]] if "COUNT" in meta else [1] * len(fields)
    if not len(fields) == len(sizes) == len(types) == len(counts):
        raise ValueError("PCD FIELDS, SIZE, TYPE and COUNT differ in length")
    for name, s, t, c in zip(fields, sizes, types, counts):
        if s not in (1, 2, 4, 8) or t not in ("I", "U", "F") or (t == "F" and s < 4) or c < 1:
            raise ValueError("PCD field %s: TYPE %s SIZE %d COUNT %d is not a field" % (name, t, s, c))
    data = meta["DATA"][0]
    if data not in ("binary", "ascii"):
        raise ValueError("unsupported PCD DATA %s" % data)  # binary_compressed names itself here
    offsets = [int(o) for o in np.cumsum([0] + [s * c for s, c in zip(sizes, counts)])]
    return PcdLayout(fields, sizes, types, counts, offsets[-1], offsets[:-1], int(meta["POINTS"][0]), data)


def pcd_is_words(layout):
    """every field 4 bytes with COUNT 1: the dialect read_pcd_header knows"""
    return all(s == 4 for s in layout.sizes) and all(c == 1 for c in layout.counts)


def pcd_slots(layout):
    """-> offsets, types (per slot of SLOTS), colour kind of a PcdLayout: x y z, and rgb / rgba as one packed word"""
    offsets, types = [-1] * 7, [REC_U8] * 7

    def put(slot, name):
        k = layout.fields.index(name)
        if (layout.types[k], layout.sizes[k]) not in _PCD_CODES:
            raise ValueError("PCD field %s: TYPE %s SIZE %d is not supported" % (name, layout.types[k], layout.sizes[k]))
        offsets[slot], types[slot] = layout.offsets[k], _PCD_CODES[layout.types[k], layout.sizes[k]]
        return k

    for slot, name in enumerate("xyz"):
        if name not in layout.fields:
            raise ValueError("a PCD without %s" % name)
        put(slot, name)
    for name in ("rgb", "rgba"):
        if name in layout.fields:
            k = put(3, name)
            if layout.sizes[k] != 4 or layout.counts[k] != 1:
                raise ValueError("PCD field %s is not one 4-byte word" % name)
            return offsets, types, COLOUR_PACKED
    return offsets, types, COLOUR_NONE


def _pcd_columns(layout):
    """(numpy format, count, byte offset) of every field, for _read_records"""
    return [(t.lower() + str(s), c, o) for t, s, c, o in zip(layout.types, layout.sizes, layout.counts, layout.offsets)]


# ---- PLY ------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": REC_I8, "int8": REC_I8, "uchar": REC_U8, "uint8": REC_U8, "short": REC_I16, "int16": REC_I16,
              "ushort": REC_U16, "uint16": REC_U16, "int": REC_I32, "int32": REC_I32, "uint": REC_U32, "uint32": REC_U32,
              "float": REC_F32, "float32": REC_F32, "double": REC_F64, "float64": REC_F64}
PLY_FORMATS = ("binary_little_endian", "binary_big_endian", "ascii")
PLY_LABEL_NAMES = ("label", "class", "scalar_label")
PlyHeader = collections.namedtuple("PlyHeader", "format n names types offsets stride slots")


def ply_header(n, coord="float", has_colors=False, has_labels=False):
    """the header text of write_point_cloud_ply (scene_io's device writer puts the same text in front of its payload)"""
    if coord not in ("float", "double"):
        raise ValueError("coord: float or double")
    lines = ["ply", "format binary_little_endian 1.0", "comment Created by pn2", "element vertex %d" % n]
    lines += ["property %s %s" % (coord, a) for a in "xyz"]
    if has_colors:
        lines += ["property uchar %s" % c for c in ("red", "green", "blue")]
    if has_labels:
        lines.append("property int label")
    return "\n".join(lines + ["end_header"]) + "\n"


def read_ply_header(f, label_property=None):
    """f: a .ply opened "rb" -> PlyHeader: the format (one of PLY_FORMATS), the number of vertices, the name, REC_* type and byte
    offset of every vertex property, the row stride, and slots = (offsets, types, colour kind) of x y z, red green blue and
    the label (the first present of PLY_LABEL_NAMES, or label_property); f is left at the first payload byte.  The vertex element
    must come first, later elements are ignored.  A list property in vertex, a missing x / y / z, an unknown type: ValueError."""
    def line():
        raw = f.readline()
        if not raw:
            raise ValueError("truncated PLY header")
        return raw.decode("ascii", "replace").split()

    if line() != ["ply"]:
        raise ValueError("not a PLY file")
    fmt, n, names, types, element = None, None, [], [], 0
    while True:
        t = line()
        if not t or t[0] in ("comment", "obj_info"):
            continue
        if t[0] == "end_header":
            break
        if t[0] == "format":
            if len(t) != 3 or t[1] not in PLY_FORMATS or t[2] != "1.0":
                raise ValueError("unsupported PLY format %s" % " ".join(t[1:]))
            fmt = t[1]
        elif t[0] == "element":
            element += 1
            if element == 1:
                if len(t) != 3 or t[1] != "vertex":
                    raise ValueError("the first PLY element must be vertex")
                n = int(t[2])
        elif t[0] == "property":
            if element != 1:
                continue  # of a later element (faces): not read
            if len(t) != 3 or t[1] not in _PLY_TYPES:
                raise ValueError("PLY vertex property %s: a list or an unknown type" % " ".join(t[1:]))
            names.append(t[2])
            types.append(_PLY_TYPES[t[1]])
        else:
            raise ValueError("unknown PLY header line %s" % " ".join(t))
    if fmt is None or n is None:
        raise ValueError("a PLY header without format or vertex element")
    sizes = [REC_SIZES[t] for t in types]
    at = [int(o) for o in np.cumsum([0] + sizes)]
    offsets, slot_types = [-1] * 7, [REC_U8] * 7

    def put(slot, name):
        offsets[slot], slot_types[slot] = at[names.index(name)], types[names.index(name)]

    for slot, name in enumerate("xyz"):
        if name not in names:
            raise ValueError("a PLY without a vertex property %s" % name)
        put(slot, name)
    colour_kind = COLOUR_NONE
    if all(c in names for c in ("red", "green", "blue")):
        colour_kind = COLOUR_THREE
        for slot, name in zip((3, 4, 5), ("red", "green", "blue")):
            put(slot, name)
            if slot_types[slot] not in _CHANNEL_TYPES:
                raise ValueError("PLY colour property %s is not uchar, ushort, float or double" % name)
    if label_property is not None and label_property not in names:
        raise ValueError("a PLY without the label property %s" % label_property)
    for name in ([label_property] if label_property is not None else PLY_LABEL_NAMES):
        if name in names:
            put(6, name)
            break
    return PlyHeader(fmt, n, names, types, at[:-1], at[-1], (offsets, slot_types, colour_kind))


def write_point_cloud_ply(path, points, colors=None, labels=None, coord="float"):
    """a binary little-endian PLY: x y z as float ((float)p) or double, optionally uchar red green blue (a uint8 colour as it
    is, a float64 colour c as clip(floor(c * 255.0), 0, 255), a NaN as 0), optionally int label -- tightly packed in that order."""
    points = np.asarray(points)
    n = len(points)
    names, formats = ["x", "y", "z"], ["<f4" if coord == "float" else "<f8"] * 3
    if colors is not None:
        names, formats = names + ["red", "green", "blue"], formats + ["u1"] * 3
    if labels is not None:
        names, formats = names + ["label"], formats + ["<i4"]
    rec = np.zeros(n, np.dtype({"names": names, "formats": formats}))  # packed: no padding
    with np.errstate(over="ignore", invalid="ignore"):
        for k, a in enumerate("xyz"):
            rec[a] = points[:, k]
        if colors is not None:
            c = np.asarray(colors)
            if c.dtype != np.uint8:
                c = np.nan_to_num(np.clip(np.floor(c.astype(np.float64) * 255.0), 0, 255), nan=0.0).astype(np.uint8)
            for k, a in enumerate(("red", "green", "blue")):
                rec[a] = c[:, k]
        if labels is not None:
            rec["label"] = np.asarray(labels).astype(np.int32)
    with open(path, "wb") as f:
        f.write(ply_header(n, coord, colors is not None, labels is not None).encode())
        f.write(rec.tobytes())


def read_point_cloud_ply(path, want_labels=False, label_property=None):
    """-> points (n,3) float64, colors (n,3) float64 (zeros without red green blue) [, labels (n,) int32 with want_labels], by
    the rules of unpack_records; binary of either byte order and ascii."""
    with open(path, "rb") as f:
        h = read_ply_header(f, label_property)
        offsets, types, colour_kind = h.slots
        if want_labels and offsets[6] < 0:
            raise ValueError("a PLY without a label property (one of %s)" % ", ".join(PLY_LABEL_NAMES))
        columns = [(REC_NUMPY[t], 1, o) for t, o in zip(h.types, h.offsets)]
        raw = _read_records(f, h.n, h.stride, columns, h.format == "ascii", "PLY")
    points, colors, labels, _ = unpack_records(raw, h.n, h.stride, offsets, types, colour_kind,
                                               big=h.format == "binary_big_endian", want_labels=want_labels)
    return (points, colors, labels) if want_labels else (points, colors)


def scene_path(stem):
    """the scene file of `stem`: <stem>.pcd where it exists, else <stem>.ply where that exists, else <stem>.pcd"""
    if not os.path.exists(stem + ".pcd") and os.path.exists(stem + ".ply"):
        return stem + ".ply"
    return stem + ".pcd"


def read_point_cloud(path):
    """read_point_cloud_pcd or read_point_cloud_ply by the extension of path (.pcd / .ply in either case)"""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".pcd", ".ply"):
        raise ValueError("a scene file is .pcd or .ply, got %s" % path)
    return read_point_cloud_pcd(path) if ext == ".pcd" else read_point_cloud_ply(path)
