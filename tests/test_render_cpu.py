"""CPU tests of the renderer (csrc/pn2_render.hip, render.py): the numpy model of the rules (tests/render_ref.py) against a naive
loop, the header's prototypes and the binding, every refusal of the three entry points with placeholder pointers, the PNG writer
parsed back, the colour table against the reference's, and -- from the model -- that the clouds the GPU test splats really hold
the edges they are named after.  Nothing here needs a GPU."""
import ctypes
import json
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as R  # noqa: E402

ARGS = {
    "pn2_label_colors": ("n", "num_class", "labels", "palette", "colors", "bad", "stream"),
    "pn2_render_splat": ("n", "index0", "points", "points_f64", "view", "perspective", "width", "height", "size", "zbuf", "culled",
                         "stream"),
    "pn2_render_resolve": ("width", "height", "zbuf", "npoints", "colors", "background", "image", "depth", "index", "stream"),
}


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _naive(points, view, width, height, size, index0, perspective, zbuf):
    """point by point, pixel by pixel, in python floats (float64) and python integers"""
    m = [[float(x) for x in row] for row in np.asarray(view, dtype=np.float64).reshape(3, 4)]
    culled = 0
    for i, (x, y, z) in enumerate(np.asarray(points).astype(np.float64).tolist()):
        t = [((row[0] * x + row[1] * y) + row[2] * z) + row[3] for row in m]
        u, v, d = t
        if perspective:
            if not d > 0:
                culled += 1
                continue
            u, v = t[0] / d, t[1] / d
        if not (math.isfinite(u) and math.isfinite(v) and math.isfinite(d) and -R.LIMIT <= u < R.LIMIT and -R.LIMIT <= v < R.LIMIT):
            culled += 1
            continue
        px, py = math.floor(u), math.floor(v)
        with np.errstate(over="ignore"):
            f = np.float32(d) + np.float32(0.0)
        bits = struct.unpack("<I", struct.pack("<f", f))[0]
        k = (~bits & 0xFFFFFFFF) if bits >> 31 else bits | 0x80000000
        key = (k << 32) | (index0 + i)
        drawn = False
        for b in range(size):
            for a in range(size):
                qx, qy = px - size // 2 + a, py - size // 2 + b
                if 0 <= qx < width and 0 <= qy < height:
                    drawn = True
                    zbuf[qy * width + qx] = min(zbuf[qy * width + qx], key)
        culled += not drawn
    return culled


@pytest.mark.parametrize("perspective", [False, True])
@pytest.mark.parametrize("size", [1, 2, 3, 8])
def test_model_equals_a_naive_loop(size, perspective):
    rs = np.random.RandomState(size * 2 + perspective)
    w, h, n = 13, 9, 300
    pts = rs.uniform(-2.0, 2.0, (n, 3))
    pts[::7] = np.round(pts[::7])  # integer coordinates: pixel boundaries and depth ties
    pts[5], pts[6, 1], pts[7, 2] = np.nan, np.inf, -0.0
    view = np.array([[3.0, 0.5, 0.0, 6.0], [0.0, -2.5, 0.25, 4.0], [0.0, 0.0, 1.0, 0.5 if perspective else 0.0]])
    zbuf = R.empty(w, h)
    naive = [int(R.EMPTY)] * (w * h)
    for lo, hi in ((0, 100), (100, 300)):  # two calls into one buffer
        got = R.splat(zbuf, pts[lo:hi], view, w, h, size, lo, perspective)
        assert got == _naive(pts[lo:hi], view, w, h, size, lo, perspective, naive)
    assert zbuf.tolist() == naive and (zbuf != R.EMPTY).any() and (size > 1 or (zbuf == R.EMPTY).any())
    image, depth, index = R.resolve(zbuf, w, h, np.arange(3 * n).reshape(n, 3) % 251, (9, 8, 7))
    for p, key in enumerate(naive):
        y, x = divmod(p, w)
        if key == int(R.EMPTY):
            assert index[y, x] == -1 and depth[y, x] == np.inf and image[y, x].tolist() == [9, 8, 7]
        else:
            i = key & 0xFFFFFFFF
            d = ((view[2, 0] * pts[i, 0] + view[2, 1] * pts[i, 1]) + view[2, 2] * pts[i, 2]) + view[2, 3]
            assert index[y, x] == i and depth[y, x] == np.float32(d) and image[y, x].tolist() == [(3 * i + c) % 251 for c in range(3)]


def test_depth_keys_keep_the_order_of_float32():
    f = np.array([-np.inf, -3e38, -1.0, -1e-45, 0.0, 1e-45, 1.0, 3e38, np.inf], dtype=np.float32)
    k = R.depth_key(f.astype(np.float64))
    assert (np.diff(k.astype(np.int64)) > 0).all() and k.max() < 0xFFFFFFFF
    assert R.key_depth(k).tobytes() == f.tobytes()
    assert R.depth_key(np.array([-0.0]))[0] == R.depth_key(np.array([0.0]))[0] == 0x80000000


def test_label_colors_model():
    c, bad = R.label_colors([0, 8, -1, 9, 3], R_PALETTE())
    assert bad == 2 and c.tolist() == [[255, 255, 255], [128, 128, 0], [0, 0, 0], [0, 0, 0], [255, 0, 255]]


def R_PALETTE():
    with open(os.path.join(ROOT, "tests", "golden", "label_colors.json")) as f:
        return json.load(f)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS
    i, p = ctypes.c_int, ctypes.c_void_p
    assert fns["pn2_label_colors"].argtypes == [i, i, p, p, p, p, p]
    assert fns["pn2_render_splat"].argtypes == [i, i, p, i, p, i, i, i, i, p, p, p]
    assert fns["pn2_render_resolve"].argtypes == [i, i, p, i, p, p, p, p, p, p]
    assert "pn2_render_splat" in pn2._lib._STATEFUL  # it takes the minimum into the caller's z-buffer
    assert not {"pn2_label_colors", "pn2_render_resolve"} & pn2._lib._STATEFUL
    assert pn2._lib.ABI.constants["PN2_ABI_VERSION"] == 2 and pn2._lib.lib.pn2_abi_version() == 2
    lib = ctypes.CDLL(pn2._lib.LIB_PATH)
    for name in ARGS:
        assert hasattr(lib, name), name
    assert "pn2_render.hip" in pn2._lib._build.SOURCES


def _caller(pn2, name, good):
    names = pn2._lib.ABI.functions[name].argnames

    def call(**change):
        a = dict(good, **change)
        return getattr(pn2._lib.lib, name)(*[a[k] for k in names])
    return call


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL, ERANGE, EUNSUP = K["PN2_EINVAL"], K["PN2_ENULL"], K["PN2_ERANGE"], K["PN2_EUNSUP"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    view = (ctypes.c_double * 12)(*R.IDENTITY.reshape(-1))
    bg = (ctypes.c_uint8 * 3)(1, 2, 3)

    col = _caller(pn2, "pn2_label_colors", dict(n=100, num_class=9, labels=fake, palette=fake, colors=fake, bad=fake, stream=None))
    for bad in (dict(n=0), dict(n=-1), dict(num_class=0), dict(num_class=-3)):
        assert col(**bad) == EINVAL, bad
    assert col(num_class=257) == EUNSUP
    for required in ("labels", "palette", "colors"):
        assert col(**{required: None}) == ENULL, required
    assert col(labels=odd(2)) == EINVAL and col(bad=odd(4)) == EINVAL
    # the order: sizes, num_class, NULL, alignment
    assert col(n=0, num_class=257) == EINVAL and col(num_class=257, labels=None) == EUNSUP and col(colors=None, labels=odd(2)) == ENULL

    splat = _caller(pn2, "pn2_render_splat", dict(n=100, index0=0, points=fake, points_f64=0, view=view, perspective=0, width=64,
                                                  height=48, size=1, zbuf=fake, culled=fake, stream=None))
    for bad in (dict(n=0), dict(n=-5), dict(width=0), dict(width=-1), dict(height=0), dict(height=-1), dict(size=0), dict(size=-1),
                dict(points_f64=2), dict(perspective=-1)):
        assert splat(**bad) == EINVAL, bad
    assert splat(size=17) == EUNSUP and splat(size=16, points=None) == ENULL
    assert splat(index0=-1) == ERANGE
    assert splat(index0=2 ** 31 - 100, n=100) == ERANGE and splat(index0=2 ** 31 - 101, n=100, points=None) == ENULL
    assert splat(width=1 << 16, height=1 << 15) == ERANGE and splat(width=(1 << 16) - 1, height=1 << 15, zbuf=None) == ENULL
    for required in ("points", "view", "zbuf"):
        assert splat(**{required: None}) == ENULL, required
    assert splat(zbuf=odd(1)) == EINVAL and splat(zbuf=odd(4)) == EINVAL and splat(culled=odd(4)) == EINVAL
    assert splat(points=odd(2)) == EINVAL and splat(points=odd(4), points_f64=1) == EINVAL
    # the order: sizes, ranges, size > 16, NULL, alignment
    assert splat(n=0, index0=-1, size=17) == EINVAL and splat(index0=-1, size=17) == ERANGE
    assert splat(size=17, zbuf=None) == EUNSUP and splat(zbuf=None, points=odd(2)) == ENULL

    res = _caller(pn2, "pn2_render_resolve", dict(width=64, height=48, zbuf=fake, npoints=100, colors=fake, background=bg,
                                                  image=fake, depth=fake, index=fake, stream=None))
    for bad in (dict(width=0), dict(height=0), dict(height=-2), dict(npoints=-1)):
        assert res(**bad) == EINVAL, bad
    assert res(width=1 << 16, height=1 << 15) == ERANGE
    assert res(zbuf=None) == ENULL and res(image=None, depth=None, index=None) == ENULL
    assert res(colors=None) == ENULL and res(background=None) == ENULL  # an image needs both
    assert res(zbuf=odd(4)) == EINVAL and res(depth=odd(2)) == EINVAL and res(index=odd(1)) == EINVAL
    assert res(width=0, zbuf=None) == EINVAL and res(width=1 << 16, height=1 << 15, zbuf=None) == ERANGE
    assert res(zbuf=None, depth=odd(2)) == ENULL


def test_python_side_checks_come_before_the_device(pn2):
    import torch
    r = pn2.render
    with pytest.raises(ValueError, match="MI355X only"):
        r.colorize_point_cloud(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="MI355X only"):
        r.Renderer(8, 8, device="cpu")
    with pytest.raises(ValueError, match="size"):
        r.Renderer(8, 8, size=17)
    with pytest.raises(ValueError, match="MI355X only"):
        r.fit_view(torch.zeros(4, 3))
    assert callable(r.render_labels) and callable(r.render_colors) and r.VIEWS == ("top", "front", "side", "iso")


# ---- the image writers -----------------------------------------------------------------------------------------------------------
def _parse_png(raw):
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        length, kind = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + length]
        crc, = struct.unpack(">I", raw[at + 8 + length:at + 12 + length])
        assert crc == zlib.crc32(kind + data) & 0xFFFFFFFF, kind
        chunks.append((kind, data))
        at += 12 + length
    assert at == len(raw)
    return chunks


@pytest.mark.parametrize("w, h", [(1, 1), (7, 5), (257, 3)])
def test_png_is_parsed_back(pn2, tmp_path, w, h):
    img = np.random.RandomState(w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    pn2.render.write_png(path, img)
    with open(path, "rb") as f:
        chunks = _parse_png(f.read())
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (w, h, 8, 2, 0, 0, 0)  # 8-bit RGB, deflate, adaptive filtering, no interlace
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all() and rows[:, 1:].tobytes() == img.tobytes()  # filter type 0: the bytes themselves
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.asarray(im), img)
    import torch
    pn2.render.write_png(path, torch.from_numpy(img))  # a tensor gives the same file
    with open(path, "rb") as f:
        assert _parse_png(f.read()) == chunks
    ppm = str(tmp_path / "a.ppm")
    pn2.render.write_ppm(ppm, img)
    with open(ppm, "rb") as f:
        assert f.read() == b"P6\n%d %d\n255\n" % (w, h) + img.tobytes()
    for bad in (img[:, :, :2], img.astype(np.int32), img[:0]):
        with pytest.raises(ValueError):
            pn2.render.write_png(path, bad)


# ---- the colours -----------------------------------------------------------------------------------------------------------------
def test_label_colors_are_the_reference_table(pn2):
    table = R_PALETTE()
    assert len(table) == 9 and [list(c) for c in pn2.render.LABEL_COLORS] == table
    # a uint8 colour c reaches a file as the float64 c / 255.0 of the host writers and comes back as floor(that * 255.0): itself
    c = np.arange(256)
    assert (np.floor((c / 255.0) * 255.0) == c).all()


# ---- the edges the GPU test claims -------------------------------------------------------------------------------------------------
def test_edge_cloud_holds_its_edges():
    E, w, h = R.EDGE, R.EDGE_W, R.EDGE_H
    pts = R.edge_cloud()
    assert len(pts) == len(E)
    u, v, d, ok = R.project(pts, R.EDGE_VIEW)
    px, py, k, _ = R.pixels(pts, R.EDGE_VIEW)
    # culled in floating point: NaN, +-inf, 1e30; a depth of 1e300 is finite and drawn at float32 +inf
    assert not ok[[E["nan"], E["plus_inf"], E["minus_inf"], E["huge"]]].any() and ok.sum() == len(pts) - 4
    assert ok[E["huge_depth"]] and k[E["huge_depth"]] == 0xFF800000
    # the tie: one pixel, one key word -> the lower index
    assert (px[E["tie_a"]], py[E["tie_a"]], k[E["tie_a"]]) == (px[E["tie_b"]], py[E["tie_b"]], k[E["tie_b"]])
    # equal only after the float32 rounding, and the farther float64 depth holds the lower index
    assert d[E["round_a"]] > d[E["round_b"]] and k[E["round_a"]] == k[E["round_b"]] and px[E["round_a"]] == px[E["round_b"]]
    assert u[E["u_zero"]] == 0 and not np.signbit(u[E["u_zero"]]) and px[E["u_zero"]] == 0
    assert u[E["u_minus_zero"]] == 0 and np.signbit(u[E["u_minus_zero"]]) and px[E["u_minus_zero"]] == 0
    assert u[E["u_width"]] == w and px[E["u_width"]] == w
    assert u[E["u_below_zero"]] == np.nextafter(0.0, -1.0) and px[E["u_below_zero"]] == -1
    assert np.signbit(d[E["zero_minus"]]) and not np.signbit(d[E["zero_plus"]]) and k[E["zero_minus"]] == k[E["zero_plus"]] == 0x80000000
    assert E["zero_plus"] < E["zero_minus"]  # without the + 0.0f the key of -0 would be the smaller and win
    assert k[E["neg_near"]] < k[E["neg_far"]] < 0x80000000 and E["neg_near"] < E["neg_far"]

    z1 = R.empty(w, h)
    culled1 = R.splat(z1, pts, R.EDGE_VIEW, w, h, 1)
    _, _, index = R.resolve(z1, w, h)
    assert culled1 == 6  # the four above, u = width and u just below 0
    assert index[2, 3] == E["tie_a"] and index[2, 4] == E["round_a"] and index[1, 0] == E["u_zero"] and index[3, 0] == E["u_minus_zero"]
    assert index[4, 1] == E["zero_plus"] and index[4, 2] == E["neg_near"]
    assert E["u_width"] not in index and E["u_below_zero"] not in index

    # size 3: every corner splat keeps 4 of its 9 pixels, and the two points just outside reach the image's edge columns
    z3 = R.empty(w, h)
    assert R.splat(z3, pts, R.EDGE_VIEW, w, h, 3) == 4
    _, _, index = R.resolve(z3, w, h)
    for name, ys, xs in (("corner_00", (0, 1), (0, 1)), ("corner_w0", (0, 1), (w - 2, w - 1)), ("corner_0h", (h - 2, h - 1), (0, 1)),
                         ("corner_wh", (h - 2, h - 1), (w - 2, w - 1))):
        seen = {(y, x) for y, x in zip(*np.nonzero(index == E[name]))}
        assert seen == {(y, x) for y in ys for x in xs}, name  # the nearest points of the cloud: nothing hides them
    assert E["u_below_zero"] in index[:, 0] and E["u_width"] in index[:, w - 1]
    # size 2 covers px - 1 .. px: the point at u = width reaches the last column, the one at -1 nothing
    z2 = R.empty(w, h)
    R.splat(z2, pts, R.EDGE_VIEW, w, h, 2)
    _, _, index = R.resolve(z2, w, h)
    assert E["u_width"] in index[:, w - 1] and E["u_below_zero"] not in index


def test_perspective_cloud_holds_its_edges():
    P, w, h = R.PERSPECTIVE, R.EDGE_W, R.EDGE_H
    pts = R.perspective_cloud()
    u, v, d, ok = R.project(pts, R.PINHOLE, True)
    assert ok.tolist() == [True, True, False, False, False, False, False]
    assert d[P["d_zero"]] == 0 and d[P["d_negative"]] < 0 and d[P["d_minus_zero"]] == 0
    assert np.isnan(v[P["nan"]]) and d[P["wide"]] > 0 and u[P["wide"]] >= R.LIMIT
    z = R.empty(w, h)
    assert R.splat(z, pts, R.PINHOLE, w, h, 1, 0, True) == 5
    _, depth, index = R.resolve(z, w, h)
    assert index[3, 4] == P["ahead"] and depth[3, 4] == 1.0 and (index >= 0).sum() == 1  # both on the axis: the nearer one
