"""The numpy model of the renderer's rules (include/pn2_abi.h: pn2_label_colors, pn2_render_splat, pn2_render_resolve), restated
one elementwise float64 operation at a time in the stated association, and the edge-case clouds the CPU and the GPU tests share.
Everything is compared for equality: the z-buffer is a per-pixel minimum over integer keys."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LIMIT = 2.0 ** 30


def label_colors(labels, palette):
    """-> colors (n,3) uint8, the count of labels outside the palette"""
    labels = np.asarray(labels, dtype=np.int32)
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    bad = (labels < 0) | (labels >= len(palette))
    colors = palette[np.where(bad, 0, labels)]
    colors[bad] = 0
    return colors, int(bad.sum())


def project(points, view, perspective=False):
    """-> u, v, d (float64), ok: the points that survive the floating-point culling"""
    p = np.asarray(points).astype(np.float64)
    m = np.asarray(view, dtype=np.float64).reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        t = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]
        d = t[2]
        if perspective:
            u, v, ok = t[0] / d, t[1] / d, d > 0
        else:
            u, v, ok = t[0], t[1], np.ones(len(p), dtype=bool)
        ok = ok & np.isfinite(u) & np.isfinite(v) & np.isfinite(d) & (u >= -LIMIT) & (u < LIMIT) & (v >= -LIMIT) & (v < LIMIT)
    return u, v, d, ok


def depth_key(d):
    """float64 depths -> the order-preserving uint32 image of f = (float)d + 0.0f"""
    with np.errstate(over="ignore"):
        f = np.asarray(d, dtype=np.float64).astype(np.float32) + np.float32(0.0)
    b = f.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_depth(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def pixels(points, view, perspective=False):
    """-> px, py (int64; 0 where culled), key high words (uint32), ok"""
    u, v, d, ok = project(points, view, perspective)
    px = np.floor(np.where(ok, u, 0.0)).astype(np.int64)
    py = np.floor(np.where(ok, v, 0.0)).astype(np.int64)
    return px, py, depth_key(np.where(ok, d, 0.0)), ok


def splat(zbuf, points, view, width, height, size=1, index0=0, perspective=False):
    """takes the keys of the points into zbuf ((height*width,) uint64, in place) -> the number of points culled"""
    assert zbuf.dtype == np.uint64 and zbuf.shape == (height * width,)
    px, py, k, ok = pixels(points, view, perspective)
    key = (k.astype(np.uint64) << np.uint64(32)) | (np.arange(len(px), dtype=np.uint64) + np.uint64(index0))
    drawn = np.zeros(len(px), dtype=bool)
    for b in range(size):
        for a in range(size):
            x, y = px - size // 2 + a, py - size // 2 + b
            inside = ok & (x >= 0) & (x < width) & (y >= 0) & (y < height)
            np.minimum.at(zbuf, (y * width + x)[inside], key[inside])
            drawn |= inside
    return int((~drawn).sum())


def empty(width, height):
    return np.full((height * width,), EMPTY, dtype=np.uint64)


def resolve(zbuf, width, height, colors=None, background=(0, 0, 0)):
    """-> image (H,W,3) uint8 (None without colors), depth (H,W) float32, index (H,W) int32"""
    is_empty = zbuf == EMPTY
    low = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    index = np.where(is_empty, -1, low).astype(np.int32)
    depth = np.where(is_empty, np.float32(np.inf), key_depth((zbuf >> np.uint64(32)).astype(np.uint32))).astype(np.float32)
    image = None
    if colors is not None:
        colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
        has = ~is_empty & (low < len(colors))
        image = np.empty((height * width, 3), dtype=np.uint8)
        image[:] = np.asarray(background, dtype=np.uint8)
        image[has] = colors[low[has]]
        image = image.reshape(height, width, 3)
    return image, depth.reshape(height, width), index.reshape(height, width)


# ---- the edge-case clouds ------------------------------------------------------------------------------------------------------
EDGE_W, EDGE_H = 8, 6
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)  # u = x, v = y, d = z
# the same with minus zeros in the first and the last row, so that x = -0.0 reaches u and z = -0.0 reaches d as -0.0 (for the
# positive x and y of those points; any +0 term would turn the sum into +0)
EDGE_VIEW = np.array([[1, -0.0, -0.0, -0.0], [0, 1, 0, 0], [-0.0, -0.0, 1, -0.0]], dtype=np.float64)
# a pinhole camera at the origin looking along +z: u = (2x + 4z) / z, v = (2y + 3z) / z
PINHOLE = np.array([[2, 0, 4, 0], [0, 2, 3, 0], [0, 0, 1, 0]], dtype=np.float64)
EDGE = {name: i for i, name in enumerate((
    "tie_a", "tie_b",                      # the same pixel and depth: the lower index wins
    "round_a", "round_b",                  # float64 depths 1 + 2^-40 and 1: equal as float32, so round_a (lower index) wins
    "u_zero", "u_minus_zero", "u_width", "u_below_zero",
    "zero_plus", "zero_minus",             # depths +0.0 then -0.0 on one pixel: -0 becomes +0, the lower index wins
    "neg_near", "neg_far",                 # depths -3 and -2: the negative keys keep their order
    "corner_00", "corner_w0", "corner_0h", "corner_wh",  # depth -5, the nearest of the cloud: a size x size splat clipped at a corner
    "nan", "plus_inf", "minus_inf", "huge", "huge_depth"))}


def edge_cloud():
    """(21,3) float64 for EDGE_VIEW on an EDGE_W x EDGE_H image; rows named by EDGE"""
    nan, inf = np.nan, np.inf
    return np.array([
        [3.5, 2.5, 1.0], [3.5, 2.5, 1.0],
        [4.5, 2.5, 1.0 + 2.0 ** -40], [4.5, 2.5, 1.0],
        [0.0, 1.5, 2.0], [-0.0, 3.5, 2.0], [float(EDGE_W), 1.5, 1.5], [np.nextafter(0.0, -1.0), 2.5, 1.5],
        [1.5, 4.5, 0.0], [1.5, 4.5, -0.0],
        [2.5, 4.5, -3.0], [2.5, 4.5, -2.0],
        [0.5, 0.5, -5.0], [EDGE_W - 0.5, 0.5, -5.0], [0.5, EDGE_H - 0.5, -5.0], [EDGE_W - 0.5, EDGE_H - 0.5, -5.0],
        [nan, 1.0, 1.0], [1.0, inf, 1.0], [-inf, 1.0, 1.0], [1e30, 1.0, 1.0], [5.5, 3.5, 1e300]], dtype=np.float64)


PERSPECTIVE = {name: i for i, name in enumerate(("ahead", "ahead_far", "d_zero", "d_negative", "d_minus_zero", "nan", "wide"))}


def perspective_cloud():
    """(7,3) float64 for PINHOLE on an EDGE_W x EDGE_H image"""
    return np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 4.0], [1.0, 1.0, 0.0], [1.0, 1.0, -2.0], [0.0, 0.0, -0.0], [0.0, np.nan, 1.0],
                     [1e6, 0.0, 1e-3]], dtype=np.float64)
