"""A headless renderer: a point cloud with per-point colours or labels becomes an RGB image on the device, where the reference
opens an Open3D window (visualize.py, kitti_visualize.py) and colours a cloud on the host (colorize.py,
util/point_cloud_util.py:colorize_point_cloud).  The kernels are csrc/pn2_render.hip; the rules are in include/pn2_abi.h
(pn2_render_splat) and tests/render_ref.py is their numpy model.

    colors = colorize_point_cloud(labels)                        # (n,3) uint8 from the reference's nine colours
    view = fit_view(points, "top", width=1920, height=1080)      # 3x4 float64: the cloud's box fitted into the image
    r = Renderer(1920, 1080, size=2)
    r.clear(); r.splat(points, view); img = r.image(colors)      # (H,W,3) uint8 on the device; r.depth(), r.indices(), r.culled
    write_png("scene.png", img)                                  # zlib and struct only
    img = render_labels(points, labels, view="iso")              # one call

The z-buffer is one 64-bit atomic minimum per pixel touched, (ordered float32 depth << 32) | point index: nearest depth, then lowest
index, whatever the order of arrival.  A Renderer allocates its buffers once; clear / splat / image are launches and fills without
a host synchronisation, so a frame loop reuses them and a frame can be captured into a graph.
"""
import ctypes
import math
import struct
import zlib

import numpy as np
import torch

from ._lib import launch, ptr, require_cuda

# util/point_cloud_util.py:6-16 of the reference: label -> colour
LABEL_COLORS = ((255, 255, 255), (0, 0, 255), (128, 0, 0), (255, 0, 255), (0, 128, 0), (255, 0, 0), (128, 0, 128), (0, 0, 128),
                (128, 128, 0))
MAX_SIZE = 16
VIEWS = ("top", "front", "side", "iso")


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("pn2.render runs on the MI355X only: got device %s" % dev)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _palette(palette, dev):
    table = np.ascontiguousarray(np.asarray(palette.cpu() if torch.is_tensor(palette) else palette))
    if table.ndim != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= 256:
        raise ValueError("palette: (num_class <= 256, 3)")
    if table.dtype != np.uint8:
        if table.dtype.kind not in "iu" or table.min() < 0 or table.max() > 255:
            raise ValueError("palette: integers in [0, 255]")
        table = table.astype(np.uint8)
    return torch.from_numpy(table).to(dev)


def colorize_point_cloud(labels, palette=LABEL_COLORS):
    """labels (n,) integers on the device -> (n,3) uint8 = palette[labels].  A label outside the palette: ValueError, as the
    reference's dictionary fails on it (this reads one counter back)."""
    require_cuda(labels)
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("labels: (n,) integers")
    dev = labels.device
    table = _palette(palette, dev)
    n = int(labels.shape[0])
    colors = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    if n == 0:
        return colors
    if labels.dtype != torch.int32:
        lo, hi = torch.aminmax(labels)
        if int(lo) < 0 or int(hi) >= table.shape[0]:
            raise ValueError("a label outside [0, %d)" % table.shape[0])
    lab = labels.to(torch.int32).contiguous()
    bad = torch.zeros((1,), dtype=torch.int64, device=dev)
    launch("pn2_label_colors", dev, n, int(table.shape[0]), ptr(lab), ptr(table), ptr(colors), ptr(bad))
    nbad = int(bad.item())
    if nbad:
        raise ValueError("%d labels outside [0, %d)" % (nbad, table.shape[0]))
    return colors


def _view_array(view):
    m = np.asarray(view.cpu() if torch.is_tensor(view) else view, dtype=np.float64)
    if m.shape != (3, 4):
        raise ValueError("view: a 3x4 matrix")
    return (ctypes.c_double * 12)(*m.reshape(-1).tolist())


class Renderer:
    """A width x height z-buffer and its images on one device, allocated once.

        clear()                                        empty z-buffer, culled = 0
        splat(points, view, index0=0, perspective=False)   points (n,3) float32 / float64 on the device, view a 3x4 matrix (host);
                                                       call it repeatedly for chunks (index0 = the chunk's first global index)
                                                       or several clouds: the result does not depend on the order
        image(colors)  -> (H,W,3) uint8                colors (npoints,3) uint8 indexed by the global point index
        depth()        -> (H,W) float32, +inf where empty;   indices() -> (H,W) int32, -1 where empty
        culled                                         points that reached no pixel so far (reads one counter back)

    image / depth / indices return the renderer's own buffers: the next call overwrites them."""

    def __init__(self, width, height, size=1, background=(0, 0, 0), device="cuda"):
        width, height, size = int(width), int(height), int(size)
        if width <= 0 or height <= 0 or width * height >= 2 ** 31:
            raise ValueError("width, height: positive, fewer than 2^31 pixels")
        if not 1 <= size <= MAX_SIZE:
            raise ValueError("size: 1 to %d pixels" % MAX_SIZE)
        background = tuple(int(c) for c in background)
        if len(background) != 3 or min(background) < 0 or max(background) > 255:
            raise ValueError("background: three bytes")
        self.width, self.height, self.size, self.background = width, height, size, background
        self.device = dev = _device(device)
        self._bg = (ctypes.c_uint8 * 3)(*background)
        self._zbuf = torch.empty((height * width,), dtype=torch.int64, device=dev)  # the uint64 keys
        self._culled = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._image = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
        self._depth = torch.empty((height, width), dtype=torch.float32, device=dev)
        self._index = torch.empty((height, width), dtype=torch.int32, device=dev)
        self.clear()

    def clear(self):
        self._zbuf.fill_(-1)  # every bit set: empty
        self._culled.zero_()

    def splat(self, points, view, index0=0, perspective=False):
        require_cuda(points)
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype not in (torch.float32, torch.float64):
            raise ValueError("points: (n,3) float32 or float64")
        if points.device != self.device:
            raise ValueError("points on %s, the renderer on %s" % (points.device, self.device))
        n, index0 = int(points.shape[0]), int(index0)
        if index0 < 0 or index0 + n > 2 ** 31 - 1:
            raise ValueError("index0 + n must stay below 2^31 - 1")
        m = _view_array(view)
        if n == 0:
            return
        points = points.contiguous()
        launch("pn2_render_splat", self.device, n, index0, ptr(points), int(points.dtype == torch.float64), m, int(bool(perspective)),
               self.width, self.height, self.size, ptr(self._zbuf), ptr(self._culled))

    def _resolve(self, colors, image, depth, index):
        launch("pn2_render_resolve", self.device, self.width, self.height, ptr(self._zbuf), 0 if colors is None else int(colors.shape[0]),
               ptr(colors), self._bg, ptr(image), ptr(depth), ptr(index))

    def image(self, colors):
        require_cuda(colors)
        if colors.dim() != 2 or colors.shape[1] != 3 or colors.dtype != torch.uint8 or colors.device != self.device:
            raise ValueError("colors: (npoints,3) uint8 on %s" % self.device)
        # an empty table (npoints = 0, no pointer): every pixel is background
        self._resolve(colors.contiguous() if colors.shape[0] else None, self._image, None, None)
        return self._image

    def depth(self):
        self._resolve(None, None, self._depth, None)
        return self._depth

    def indices(self):
        self._resolve(None, None, None, self._index)
        return self._index

    @property
    def culled(self):
        return int(self._culled.item())


def _axes(view):
    """-> right, down, forward: the world directions of the image's u, v and depth"""
    if view == "top":      # from above, north up
        return (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)
    if view == "front":    # from -y towards +y, z up
        return (1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)
    if view == "side":     # from +x towards -x, z up
        return (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (-1.0, 0.0, 0.0)
    if view == "iso":      # from the corner (-1,-1,+1) towards (+1,+1,-1)
        s2, s3, s6 = math.sqrt(2.0), math.sqrt(3.0), math.sqrt(6.0)
        return (1 / s2, -1 / s2, 0.0), (-1 / s6, -1 / s6, -2 / s6), (1 / s3, 1 / s3, -1 / s3)
    raise ValueError("view: one of %s" % ", ".join(VIEWS))


def fit_view(points, view="top", width=1920, height=1080, margin=0.02, perspective=False, fov=60.0):
    """-> the 3x4 float64 matrix (numpy) that fits the cloud into a width x height image seen from `view`, aspect preserved, a
    `margin` fraction of each side left free; the image row grows downward and depth grows away from the viewer (0 at the nearest
    point, in world units).  The cloud's extents along the three image axes are torch reductions on the device, read back as six
    numbers in one copy; the matrix is built on the host in float64.  perspective=True: the matrix of a pinhole camera on the
    view's axis whose field of view `fov` (degrees, the smaller image side) holds the box's sphere -- for
    splat(..., perspective=True).  Points are taken to be finite."""
    require_cuda(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
        raise ValueError("points: (n > 0, 3)")
    if not 0.0 <= margin < 0.5:
        raise ValueError("margin: in [0, 0.5)")
    axes = np.array(_axes(view), dtype=np.float64)
    p = points.to(torch.float64)
    ext = []
    for a in axes:
        q = (p[:, 0] * a[0] + p[:, 1] * a[1]) + p[:, 2] * a[2]
        ext += [q.amin(), q.amax()]
    ulo, uhi, vlo, vhi, dlo, dhi = torch.stack(ext).cpu().tolist()  # the one host read
    usable_w, usable_h = width * (1.0 - 2.0 * margin), height * (1.0 - 2.0 * margin)
    cu, cv = 0.5 * (ulo + uhi), 0.5 * (vlo + vhi)
    m = np.zeros((3, 4), dtype=np.float64)
    if not perspective:
        fits = [usable / e for usable, e in ((usable_w, uhi - ulo), (usable_h, vhi - vlo)) if e > 0.0]
        s = min(fits) * (1.0 - 1e-9) if fits else 1.0  # just inside: the far edge stays below width / height at margin = 0
        m[0, :3], m[0, 3] = s * axes[0], 0.5 * width - s * cu
        m[1, :3], m[1, 3] = s * axes[1], 0.5 * height - s * cv
        m[2, :3], m[2, 3] = axes[2], -dlo
        return m
    if not 0.0 < fov < 180.0:
        raise ValueError("fov: in (0, 180) degrees")
    half = math.radians(fov) / 2.0
    radius = 0.5 * math.sqrt((uhi - ulo) ** 2 + (vhi - vlo) ** 2 + (dhi - dlo) ** 2) or 1.0
    eye_d = 0.5 * (dlo + dhi) - radius / math.sin(half)  # the camera's place on the depth axis
    focal = 0.5 * min(usable_w, usable_h) / math.tan(half)
    m[2, :3], m[2, 3] = axes[2], -eye_d
    m[0, :3], m[0, 3] = focal * axes[0] + 0.5 * width * axes[2], -focal * cu - 0.5 * width * eye_d
    m[1, :3], m[1, 3] = focal * axes[1] + 0.5 * height * axes[2], -focal * cv - 0.5 * height * eye_d
    return m


def render_colors(points, colors, view="top", width=1920, height=1080, size=1, background=(0, 0, 0), margin=0.02,
                  perspective=False, renderer=None):
    """points (n,3), colors (n,3) uint8 on the device -> the (height,width,3) uint8 image of the fitted `view` (a name of
    fit_view, or a 3x4 matrix).  renderer: reuse one (its size wins)."""
    r = renderer or Renderer(width, height, size, background, points.device)
    m = fit_view(points, view, r.width, r.height, margin, perspective) if isinstance(view, str) else view
    r.clear()
    r.splat(points, m, 0, perspective)
    return r.image(colors)


def render_labels(points, labels, view="top", palette=LABEL_COLORS, **kw):
    """render_colors of colorize_point_cloud(labels, palette)"""
    return render_colors(points, colorize_point_cloud(labels, palette), view, **kw)


def _host_image(image):
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("image: (H,W,3) uint8")
    return np.ascontiguousarray(a)


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image, level=6):
    """image: (H,W,3) uint8, a tensor or an array -> an 8-bit RGB PNG, every row with filter type 0"""
    a = _host_image(image)
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)  # a filter byte 0 in front of every row
    rows[:, 1:] = a.reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))  # 8 bits, colour type 2, no interlace
        f.write(_png_chunk(b"IDAT", zlib.compress(rows.tobytes(), level)))
        f.write(_png_chunk(b"IEND", b""))


def write_ppm(path, image):
    """image: (H,W,3) uint8 -> a binary PPM (P6)"""
    a = _host_image(image)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())
