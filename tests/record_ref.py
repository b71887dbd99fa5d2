"""Host model of the record kernels (csrc/pn2_records.hip), written from the rules of include/pn2_abi.h "records", not from the
kernels: rows of any byte stride with typed fields at any byte offset, unpacked and packed in numpy through a structured dtype
built from the seven slots.  Also the case lists the CPU and GPU tests share."""
import numpy as np

import scene_io_ref as S

U8, I8, U16, I16, U32, I32, F32, F64 = range(8)
SIZES = (1, 1, 2, 2, 4, 4, 4, 8)
NUMPY = ("u1", "i1", "u2", "i2", "u4", "i4", "f4", "f8")
NONE, THREE, PACKED = range(3)
X, Y, Z, C0, C1, C2, LABEL = range(7)
ABSENT = [-1] * 7
NS = (1, 63, 64, 65, 255, 256, 257, 1025)  # both sides of a wave, of a workgroup's 256 rows, and more than one workgroup


def unit_to_byte(c):
    """floor(c * 255.0) clipped to [0, 255]; a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        t = np.floor(np.asarray(c, dtype=np.float64) * 255.0)
    return np.where(t >= 255.0, 255, np.where(t > 0.0, t, 0)).astype(np.uint8)


def _dtype(stride, offsets, types, slots, big):
    end = ">" if big else "<"
    return np.dtype({"names": ["s%d" % k for k in slots], "formats": [end + NUMPY[types[k]] for k in slots],
                     "offsets": [offsets[k] for k in slots], "itemsize": stride})


def unpack(raw, n, stride, offsets, types, colour_kind, big=False, want_colors=True, want_labels=False):
    """-> points (n,3) float64, colors (n,3) float64 or None, labels (n,) int32 or None, the number of invalid labels"""
    types = list(types)
    if colour_kind == PACKED:
        types[C0] = U32  # the word's bits, whatever the file calls it
    slots = [X, Y, Z] + ([C0, C1, C2][:(0, 3, 1)[colour_kind]] if want_colors else []) + ([LABEL] if want_labels else [])
    rec = np.frombuffer(raw, dtype=_dtype(stride, offsets, types, slots, big), count=n)
    f64 = lambda k: rec["s%d" % k].astype(np.float64)  # noqa: E731  (exact for every type)
    with np.errstate(invalid="ignore"):  # a signalling NaN is quieted by float32 -> float64
        points = np.stack([f64(X), f64(Y), f64(Z)], axis=1)
        colors = None
        if want_colors and colour_kind == THREE:
            div = {U8: 255.0, U16: 65535.0}
            assert all(types[k] in (U8, U16, F32, F64) for k in (C0, C1, C2))
            colors = np.stack([f64(k) / div[types[k]] if types[k] in div else f64(k) for k in (C0, C1, C2)], axis=1)
        elif want_colors and colour_kind == PACKED:
            w = rec["s%d" % C0].astype(np.uint32)
            colors = np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1).astype(np.float64) / 255.0
        elif want_colors:
            colors = np.zeros((n, 3))
        labels, invalid = None, 0
        if want_labels and types[LABEL] >= F32:
            d = f64(LABEL)
            ok = np.isfinite(d) & (d == np.floor(d)) & (d >= -2.0 ** 31) & (d <= 2.0 ** 31 - 1)
            labels, invalid = np.where(ok, d, 0.0).astype(np.int64).astype(np.int32), int((~ok).sum())
        elif want_labels:
            labels = rec["s%d" % LABEL].astype(np.int64).astype(np.uint32).view(np.int32)  # value-preserving; U32 reinterpreted
    return points, colors, labels, invalid


PACK_LAYOUTS = [(coord, has_c, has_l) for coord in ("float", "double") for has_c in (False, True) for has_l in (False, True)]


def pack_stride(coord, has_colors, has_labels):
    return (12 if coord == "float" else 24) + (3 if has_colors else 0) + (4 if has_labels else 0)


def pack(points, colors=None, labels=None, coord="float"):
    """x y z as float32 ((float)p) or float64, then three uint8 channels, then an int32 label: tightly packed, little-endian"""
    n = len(points)
    names, formats = ["x", "y", "z"], ["<f4" if coord == "float" else "<f8"] * 3
    if colors is not None:
        names, formats = names + ["r", "g", "b"], formats + ["u1"] * 3
    if labels is not None:
        names, formats = names + ["label"], formats + ["<i4"]
    rec = np.zeros(n, dtype=np.dtype({"names": names, "formats": formats}))
    assert rec.dtype.itemsize == pack_stride(coord, colors is not None, labels is not None)
    with np.errstate(over="ignore"):
        for k, a in enumerate("xyz"):
            rec[a] = np.asarray(points)[:, k]
    if colors is not None:
        c = colors if colors.dtype == np.uint8 else unit_to_byte(colors)
        for k, a in enumerate("rgb"):
            rec[a] = c[:, k]
    if labels is not None:
        rec["label"] = labels
    return rec.tobytes()


def edge_data(t, n, seed):
    """n values of type code t as the little-endian numpy array: the edges first (NaN, +-inf, -0.0, denormals and the
    extremes of a float type; the extremes of an integer type), every byte value where the type is a byte, then random bits"""
    rs = np.random.RandomState(seed)
    dt = np.dtype("<" + NUMPY[t])
    out = np.frombuffer(rs.bytes(n * dt.itemsize), dtype=dt).copy()
    if t >= F32:
        info = np.finfo(dt)
        edge = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, info.tiny, -info.tiny / 4, info.smallest_subnormal, info.max, -info.max,
                         1.0, 255.0, 0.5], dtype=dt)
    else:
        info = np.iinfo(dt)
        edge = np.array([info.min, info.max, 0, 1, info.max // 2, info.max // 2 + 1], dtype=dt)
        if dt.itemsize == 1:
            edge = np.concatenate([edge, np.arange(256).astype(dt)])
    out[:min(n, len(edge))] = edge[:n]
    return out


def make_rows(n, stride, fields, big=False, seed=0):
    """n rows of `stride` random bytes with fields [(byte offset, type code, values)] laid over them -> bytes"""
    raw = np.frombuffer(np.random.RandomState(seed).bytes(n * stride), dtype=np.uint8).reshape(n, stride).copy()
    for off, t, values in fields:
        v = np.asarray(values).astype(np.dtype(("<", ">")[big] + NUMPY[t]))
        raw[:, off:off + SIZES[t]] = v.view(np.uint8).reshape(n, SIZES[t])
    return raw.tobytes()


def slots_of(**fields):
    """x=(offset, type), ... -> offsets, types"""
    offsets, types = list(ABSENT), [U8] * 7
    for name, (off, t) in fields.items():
        k = ("x", "y", "z", "c0", "c1", "c2", "label").index(name)
        offsets[k], types[k] = off, t
    return offsets, types


def stride_cases():
    """[(stride, offsets, types, colour kind)]: the strides the kernels' forms divide at (a staged span of 256 rows up to 128
    bytes, of 64 rows up to 512, the plain form above) and the alignments the field reads divide at"""
    f3 = lambda t, at, size: dict(x=(at, t), y=(at + size, t), z=(at + 2 * size, t))  # noqa: E731
    u8 = lambda at: dict(c0=(at, U8), c1=(at + 1, U8), c2=(at + 2, U8))  # noqa: E731
    return [
        (12, *slots_of(**f3(F32, 0, 4)), NONE),
        (15, *slots_of(**f3(F32, 0, 4), **u8(12)), THREE),
        (16, *slots_of(**f3(F32, 0, 4), label=(12, I32)), NONE),
        (19, *slots_of(**f3(F32, 0, 4), **u8(12), label=(15, I32)), THREE),
        (27, *slots_of(**f3(F64, 0, 8), **u8(24)), THREE),
        (31, *slots_of(**f3(F64, 0, 8), **u8(24), label=(27, I32)), THREE),
        (33, *slots_of(c0=(0, U16), c1=(2, U16), c2=(4, U16), **f3(F64, 7, 8)), THREE),
        # every field at a multiple of its size in every row: the one-access reads of 2, 4 and 8 bytes
        (64, *slots_of(x=(2, I16), y=(8, U32), z=(16, F64), c0=(28, F32), c1=(32, F32), c2=(36, F32), label=(48, F64)), THREE),
        (500, *slots_of(**f3(F32, 101, 4), c0=(7, U32), label=(496, U16)), PACKED),  # 64 rows per staged workgroup
        (513, *slots_of(**f3(F64, 3, 8), **u8(510), label=(100, I8)), THREE),        # the first stride of the plain form
        (1024, *slots_of(**f3(F64, 993, 8), **u8(1017), label=(1020, I32)), THREE),   # fields at the very end
    ]


def case_rows(n, stride, offsets, types, big=False, seed=0):
    """rows for a case: edge data in every present slot"""
    fields = [(offsets[k], types[k], edge_data(types[k], n, seed + 7 * k)) for k in range(7) if offsets[k] >= 0]
    return make_rows(n, stride, fields, big, seed)


def pcd_head(fields, sizes, types, counts, n, data="binary"):
    j = lambda v: " ".join(str(x) for x in v)  # noqa: E731
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (j(fields), j(sizes), j(types), j(counts), n, n, data)).encode()


def general_pcd_files(n=300):
    """[(name, file bytes, stride, offsets, types, colour kind)]: double coordinates with an rgb word; 1- and 2-byte fields with
    a `_` padding field of COUNT 3; a PCL descriptor of COUNT 33 in front of the coordinates"""
    out = []
    o, t = slots_of(x=(0, F64), y=(8, F64), z=(16, F64), c0=(24, F32))
    out.append(("f64", pcd_head("x y z rgb".split(), [8, 8, 8, 4], "FFFF", [1] * 4, n), 28, o, t, PACKED))
    o, t = slots_of(x=(0, F32), y=(4, F32), z=(8, F32))
    out.append(("pad", pcd_head("x y z a _ b ring".split(), [4, 4, 4, 1, 1, 1, 2], "FFFUUIU", [1, 1, 1, 1, 3, 1, 1], n), 19, o, t, NONE))
    o, t = slots_of(x=(132, F32), y=(136, F32), z=(140, F32), c0=(144, U32))
    out.append(("fpfh", pcd_head("fpfh x y z rgba".split(), [4] * 5, "FFFFU", [33, 1, 1, 1, 1], n), 148, o, t, PACKED))
    return [(name, head + case_rows(n, stride, o, t, seed=len(name)), stride, o, t, kind) for name, head, stride, o, t, kind in out]


def ply_inputs(n, seed=0):
    rs = np.random.RandomState(seed)
    p64 = np.resize(S.point_list(), (n, 3)) * 1.0
    c64 = np.stack([np.resize(S.color_list(), n), np.resize(S.color_list()[::-1], n), np.resize(np.roll(S.color_list(), 341), n)], axis=1)
    c64[::7, 1] = np.nan
    u8 = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    labels = np.resize(np.array(S.edge_values(), dtype=np.int32), n)
    return p64, rs.uniform(-300, 300, (n, 3)).astype(np.float32), c64, u8, labels
