"""Host model of scene_io (csrc/pn2_scene_io.hip), written from the rules of include/pn2_abi.h "scene files", not from the
kernels: the text of an integer table, and the rows of a binary .pcd payload packed and unpacked in numpy."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def format_rows(values):
    """values (n,) or (n, ncols) integers -> bytes: per row the "%d" tokens separated by one space, ended by '\\n'"""
    v = np.asarray(values)
    v = v.reshape(len(v), 1) if v.ndim == 1 else v
    return b"".join(b" ".join(b"%d" % x for x in row) + b"\n" for row in v.tolist())


def edge_values():
    """0, +-1, +-9, +-(10^k - 1) and +-10^k for k = 1..9, INT32_MAX, INT32_MIN + 1, INT32_MIN"""
    out = [0, 1, -1, 9, -9]
    for k in range(1, 10):
        out += [10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)]
    return out + [INT32_MAX, INT32_MIN + 1, INT32_MIN]


def pack_rows(points, colors=None):
    """points (n,3) float32 / float64, colors None, (n,3) float64 or (n,3) uint8 -> (n, 3 or 4) uint32 words: the coordinates
    rounded to float32, the colour word (r << 16) | (g << 8) | b with r = clip(floor(c * 255.0), 0, 255) of a float64 colour"""
    with np.errstate(over="ignore"):
        xyz = np.asarray(points).astype(np.float32).view(np.uint32).reshape(-1, 3)
    if colors is None:
        return np.ascontiguousarray(xyz)
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        c8 = c.astype(np.uint32)
    else:
        assert c.dtype == np.float64
        c8 = np.clip(np.floor(c * 255.0), 0, 255).astype(np.uint32)
    word = (c8[:, 0] << 16) | (c8[:, 1] << 8) | c8[:, 2]
    return np.ascontiguousarray(np.concatenate([xyz, word[:, None].astype(np.uint32)], axis=1))


def unpack_rows(rows, fields):
    """rows (n, len(fields)) uint32, fields: names -> points (n,3) float64 (the words of x y z read as float32), colors (n,3)
    float64 = byte / 255.0 (zeros without an rgb field)"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, len(fields))
    with np.errstate(invalid="ignore"):  # a signalling NaN is quieted by the conversion
        xyz = np.stack([rows[:, fields.index(a)] for a in "xyz"], axis=1).view(np.float32).astype(np.float64)
    if "rgb" not in fields:
        return xyz, np.zeros_like(xyz)
    p = rows[:, fields.index("rgb")]
    return xyz, np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], axis=1).astype(np.float64) / 255.0


def pcd_bytes(fields, rows, data="binary"):
    """a .pcd file written by hand: FIELDS as given, every field 4 bytes, rows (n, len(fields)) uint32"""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32).reshape(-1, len(fields)))
    n, k = len(rows), len(fields)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (" ".join(fields), " ".join(["4"] * k), " ".join(["F"] * k),
                                                              " ".join(["1"] * k), n, n, data)).encode()
    return head + rows.tobytes()


def pcd_file_bytes(points, colors=None):
    """the model's x y z [rgb] file: what both writers must produce"""
    return pcd_bytes(["x", "y", "z"] + (["rgb"] if colors is not None else []), pack_rows(points, colors))


def color_list():
    """float64 colours: 0, 1, every k / 255, one ulp below and above each, -0.25 and 1.5 (the clip), a denormal"""
    k = np.arange(256, dtype=np.float64) / 255.0
    vals = np.concatenate([k, np.nextafter(k, -1.0), np.nextafter(k, 2.0), [0.0, 1.0, -0.25, 1.5, 5e-324, 1e-310]])
    return vals


def point_list():
    """float64 coordinates that test the rounding to float32: halfway cases, overflow to infinity, float32 denormals, zeros"""
    f32max = float(np.finfo(np.float32).max)
    return np.array([0.0, -0.0, 1.0, -1.0, 0.1, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, f32max,
                     f32max * (1 + 2.0 ** -25), f32max * (1 + 2.0 ** -24), 1e39, -1e39, 1e300, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149,
                     2.0 ** -150, 2.0 ** -150 * 1.0000001, 3 * 2.0 ** -150, 1e-46, -1e-42, 123456.789, -9876.54321, 1e-300],
                    dtype=np.float64)
