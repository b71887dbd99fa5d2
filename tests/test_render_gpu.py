"""GPU tests of the renderer: pn2_label_colors / pn2_render_splat / pn2_render_resolve (csrc/pn2_render.hip) against the numpy
model of the rules (tests/render_ref.py), with every output between poisoned guards and the inputs unchanged; pn2.render's
Renderer (eager and captured), fit_view, and examples/colorize.py and examples/visualize.py as subprocesses.

There is no tolerance anywhere: the projection is float64 in a fixed association without contraction, the z-buffer an integer
minimum, so z-buffers, image bytes, depth bits, indices and counts are compared for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64  # guard bytes in front of and behind every output
BLOCK = 256  # threads per workgroup of the three kernels (one point or pixel each; no grid stride)

# inexact coefficients: a contracted multiply-add would round differently from the model
ORTHO = np.array([[0.7, 0.3, 0.01, 0.5], [-0.3, 0.7, 0.013, 1.25], [0.1, -0.05, 1.0, -0.6]], dtype=np.float64)
# depth 0.25 z + 0.3 + ...: mostly in front of the camera, some behind it, some close enough to be thrown far outside
PERSP = np.array([[0.9, 0.1, 0.37, 0.2], [-0.1, 0.9, 0.29, 0.1], [0.003, 0.001, 0.25, 0.3]], dtype=np.float64)


def _guarded(torch, dev, nbytes, fill=None):
    """-> raw buffer, the view of its nbytes payload bytes (8-byte aligned: G is a multiple of 8 and so is the allocation)"""
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    if fill is not None:
        raw[G:G + nbytes] = fill
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _cloud(seed, n, w, h, dtype):
    """n points whose ORTHO / PERSP images spill over every side of a w x h image; a share on a coarse lattice (equal pixels and
    equal depths: ties that the index decides), a few non-finite"""
    rs = np.random.RandomState(seed)
    s = max(w, h)
    p = np.stack([rs.uniform(-0.6 * s, 1.6 * s, n), rs.uniform(-0.6 * s, 1.6 * s, n), rs.uniform(-2.0, 6.0, n)], 1)
    lattice = rs.random_sample(n) < 0.4
    p[lattice] = np.round(p[lattice] / 4.0) * 4.0
    if n >= 16:
        p[n // 3, 0], p[n // 2, 1], p[n // 5, 2], p[n // 7, 2] = np.nan, np.inf, -np.inf, 1e300
    with np.errstate(over="ignore"):  # 1e300 is +inf as float32: culled there, drawn at depth +inf as float64
        return np.ascontiguousarray(p.astype(dtype))


class _Frame:
    """a guarded z-buffer and a culled counter on the device, with the model's next to them"""

    def __init__(self, pn2, dev, w, h, culled0=0):
        import torch
        self.pn2, self.dev, self.w, self.h, self.torch = pn2, dev, w, h, torch
        self.raw, self.zbuf = _guarded(torch, dev, 8 * w * h, fill=0xFF)
        self.culled = torch.full((1,), culled0, dtype=torch.int64, device=dev)
        self.want, self.want_culled = R.empty(w, h), culled0

    def splat(self, pts, view, size=1, index0=0, perspective=False, model=True):
        import ctypes
        torch, lib = self.torch, self.pn2._lib
        d = torch.from_numpy(pts).to(self.dev)
        m = (ctypes.c_double * 12)(*np.asarray(view, dtype=np.float64).reshape(-1))
        lib.launch("pn2_render_splat", self.dev, len(pts), index0, lib.ptr(d), int(pts.dtype == np.float64), m, int(perspective),
                   self.w, self.h, size, lib.ptr(self.zbuf), lib.ptr(self.culled))
        torch.cuda.synchronize()
        assert d.cpu().numpy().tobytes() == pts.tobytes(), "points changed"
        if model:
            self.want_culled += R.splat(self.want, pts, view, self.w, self.h, size, index0, perspective)

    def keys(self):
        return _payload(self.raw, 8 * self.w * self.h, "zbuf").view(np.uint64)

    def check(self, what=""):
        got = self.keys()
        assert np.array_equal(got, self.want), "zbuf %s: %d pixels differ" % (what, (got != self.want).sum())
        assert int(self.culled.item()) == self.want_culled, "culled %s" % what

    def resolve(self, colors=None, background=(1, 2, 3), image=True, depth=True, index=True):
        """-> image, depth, index as arrays (None where not asked for), each checked to stay inside its guards"""
        import ctypes
        torch, lib, n = self.torch, self.pn2._lib, self.w * self.h
        before = self.keys().copy()
        d_col = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint8)).to(self.dev)
        raws = {k: _guarded(torch, self.dev, b * n) for k, b in (("image", 3), ("depth", 4), ("index", 4))}
        use = dict(image=image, depth=depth, index=index)
        lib.launch("pn2_render_resolve", self.dev, self.w, self.h, lib.ptr(self.zbuf), 0 if colors is None else len(colors),
                   lib.ptr(d_col), (ctypes.c_uint8 * 3)(*background), *[lib.ptr(raws[k][1]) if use[k] else None for k in ("image", "depth", "index")])
        torch.cuda.synchronize()
        assert np.array_equal(self.keys(), before), "resolve changed the z-buffer"
        if colors is not None:
            assert d_col.cpu().numpy().tobytes() == np.ascontiguousarray(colors, dtype=np.uint8).tobytes(), "colors changed"
        out = {}
        for k, b in (("image", 3), ("depth", 4), ("index", 4)):
            pay = _payload(raws[k][0], b * n, k)
            if not use[k]:
                assert (pay == POISON).all(), "%s written though not asked for" % k
            out[k] = pay if use[k] else None
        return (None if out["image"] is None else out["image"].reshape(self.h, self.w, 3),
                None if out["depth"] is None else out["depth"].view(np.float32).reshape(self.h, self.w),
                None if out["index"] is None else out["index"].view(np.int32).reshape(self.h, self.w))

    def check_resolve(self, npoints, what=""):
        colors = (np.arange(3 * npoints).reshape(npoints, 3) * 7 % 253).astype(np.uint8)
        image, depth, index = self.resolve(colors)
        w_image, w_depth, w_index = R.resolve(self.want, self.w, self.h, colors, (1, 2, 3))
        assert np.array_equal(index, w_index) and depth.tobytes() == w_depth.tobytes() and np.array_equal(image, w_image), what


# ---- splat ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5])
def test_splat_point_counts(pn2, cuda, n, dtype):
    w, h = 65, 33
    pts = _cloud(n, n, w, h, dtype)
    for perspective, view in ((False, ORTHO), (True, PERSP)):
        f = _Frame(pn2, cuda, w, h)
        f.splat(pts, view, 2, 0, perspective)
        f.check("n=%d perspective=%d" % (n, perspective))
        f.check_resolve(n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("w, h", [(1, 1), (7, 5), (64, 64), (65, 33), (257, 3)])
def test_splat_image_and_splat_sizes(pn2, cuda, w, h, dtype):
    n = 700
    pts = _cloud(w * 100 + h, n, w, h, dtype)
    drawn = 0
    for size in (1, 2, 3, 8, 16):
        for perspective, view in ((False, ORTHO), (True, PERSP)):
            f = _Frame(pn2, cuda, w, h)
            f.splat(pts, view, size, 0, perspective)
            f.check("size=%d perspective=%d" % (size, perspective))
            f.check_resolve(n)
            drawn += int((f.want != R.EMPTY).sum())
            assert f.want_culled > 0  # the non-finite points at least
    assert drawn > 0


@pytest.mark.parametrize("w, h", [(1, 1), (1, 64)])
def test_splat_collisions(pn2, cuda, w, h):
    """4096 points onto one pixel, and onto one column: depths on a lattice of 8 values, so most arrivals lose and many tie"""
    rs = np.random.RandomState(h)
    n = 4096
    pts = np.stack([np.full(n, 0.5), rs.uniform(0, h, n), rs.randint(0, 8, n) / 4.0 - 1.0], 1)
    f = _Frame(pn2, cuda, w, h)
    f.splat(pts, R.IDENTITY, 1)
    f.check()
    assert f.want_culled == 0 and (f.want != R.EMPTY).all()
    _, depth, index = f.resolve(None, image=False)
    nearest = pts[:, 2].min()
    if h == 1:
        assert index[0, 0] == np.flatnonzero(pts[:, 2] == nearest)[0] and depth[0, 0] == np.float32(nearest)
    f.check_resolve(n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_splat_edge_clouds(pn2, cuda, dtype):
    """the clouds whose edges tests/test_render_cpu.py asserts from the model (float32 moves two of them: the model decides)"""
    w, h = R.EDGE_W, R.EDGE_H
    with np.errstate(over="ignore"):
        pts, ppts = R.edge_cloud().astype(dtype), R.perspective_cloud().astype(dtype)
    for size in (1, 2, 3):
        f = _Frame(pn2, cuda, w, h)
        f.splat(pts, R.EDGE_VIEW, size)
        f.check("size=%d" % size)
        f.check_resolve(len(pts))
        if dtype == np.float64 and size == 1:
            E = R.EDGE
            _, _, index = f.resolve(None, image=False, depth=False)
            assert f.want_culled == 6 and index[2, 3] == E["tie_a"] and index[2, 4] == E["round_a"] and index[4, 1] == E["zero_plus"]
    f = _Frame(pn2, cuda, w, h)
    f.splat(ppts, R.PINHOLE, 1, 0, True)
    f.check("perspective")
    assert f.want_culled == 5
    f.check_resolve(len(ppts))


def test_splat_is_independent_of_order_and_chunking(pn2, cuda):
    w, h, n = 65, 33, 3000
    pts = _cloud(5, n, w, h, np.float64)
    cuts = [(0, 1000), (1000, 1001), (1001, n)]
    one, fwd, rev = (_Frame(pn2, cuda, w, h) for _ in range(3))
    one.splat(pts, ORTHO, 3)
    for lo, hi in cuts:
        fwd.splat(pts[lo:hi], ORTHO, 3, lo)
    for lo, hi in reversed(cuts):
        rev.splat(pts[lo:hi], ORTHO, 3, lo)
    for f in (one, fwd, rev):
        f.check()
    assert np.array_equal(one.keys(), fwd.keys()) and np.array_equal(one.keys(), rev.keys())


def test_splat_accumulates_into_a_used_buffer_and_counter(pn2, cuda):
    """a second cloud (float32, perspective) composited over the first (float64, orthographic); the counter starts at 2^40"""
    w, h = 64, 64
    a, b = _cloud(1, 900, w, h, np.float64), _cloud(2, 500, w, h, np.float32)
    f = _Frame(pn2, cuda, w, h, culled0=1 << 40)
    f.splat(a, ORTHO, 2)
    first = f.want.copy()
    f.splat(b, PERSP, 3, len(a), True)
    f.check()
    assert (f.want != first).any() and (f.want == first)[first != R.EMPTY].any()  # some pixels won by each cloud
    assert f.want_culled > (1 << 40)
    f.check_resolve(len(a) + len(b))
    # a NULL counter is allowed
    lib, torch = pn2._lib, f.torch
    import ctypes
    d = torch.from_numpy(a).to(cuda)
    lib.launch("pn2_render_splat", cuda, len(a), 0, lib.ptr(d), 1, (ctypes.c_double * 12)(*ORTHO.reshape(-1)), 0, w, h, 2, lib.ptr(f.zbuf), None)
    torch.cuda.synchronize()
    f.check("again, without a counter")  # the same keys again: nothing moves


# ---- resolve -------------------------------------------------------------------------------------------------------------------
def test_resolve_outputs_alone_and_together(pn2, cuda):
    w, h, n = 65, 33, 400
    f = _Frame(pn2, cuda, w, h)
    f.splat(_cloud(9, n, w, h, np.float64), ORTHO, 1)
    colors = np.random.RandomState(0).randint(0, 256, (n, 3)).astype(np.uint8)
    w_image, w_depth, w_index = R.resolve(f.want, w, h, colors, (250, 0, 7))
    assert (w_index == -1).any() and (w_index >= 0).any()
    for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 1, 1)):
        image, depth, index = f.resolve(colors if use[0] else None, (250, 0, 7), *map(bool, use))
        assert image is None or np.array_equal(image, w_image)
        assert depth is None or depth.tobytes() == w_depth.tobytes()
        assert index is None or np.array_equal(index, w_index)
    # a colour table shorter than the indices: background beyond it, never a read out of bounds
    short = colors[:n // 2]
    image, _, _ = f.resolve(short, (250, 0, 7), True, False, False)
    want, _, _ = R.resolve(f.want, w, h, short, (250, 0, 7))
    assert (w_index >= n // 2).any() and np.array_equal(image, want) and not np.array_equal(want, w_image)


# ---- colours -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_class", [1, 9, 256])
def test_label_colors_equal_the_model(pn2, cuda, num_class):
    import torch
    lib = pn2._lib
    rs = np.random.RandomState(num_class)
    palette = rs.randint(0, 256, (num_class, 3)).astype(np.uint8)
    bad = torch.full((1,), 1 << 40, dtype=torch.int64, device=cuda)
    want_bad = 1 << 40
    for n in (1, 63, 64, 65, 257, BLOCK - 1, BLOCK + 1, 1000):
        labels = rs.randint(0, num_class, n).astype(np.int32)
        if n > 1:
            labels[rs.randint(0, n, max(1, n // 10))] = rs.choice([-1, num_class, -2 ** 31, 2 ** 31 - 1], max(1, n // 10))
        d_lab, d_pal = torch.from_numpy(labels).to(cuda), torch.from_numpy(palette).to(cuda)
        raw, colors = _guarded(torch, cuda, 3 * n)
        lib.launch("pn2_label_colors", cuda, n, num_class, lib.ptr(d_lab), lib.ptr(d_pal), lib.ptr(colors), lib.ptr(bad))
        torch.cuda.synchronize()
        want, nbad = R.label_colors(labels, palette)
        want_bad += nbad
        assert np.array_equal(_payload(raw, 3 * n, "colors").reshape(n, 3), want), n
        assert int(bad.item()) == want_bad, n  # accumulates, never zeroed
        assert d_lab.cpu().numpy().tobytes() == labels.tobytes() and d_pal.cpu().numpy().tobytes() == palette.tobytes()
    assert want_bad > (1 << 40)
    lib.launch("pn2_label_colors", cuda, n, num_class, lib.ptr(d_lab), lib.ptr(d_pal), lib.ptr(colors), None)  # no counter
    torch.cuda.synchronize()
    assert np.array_equal(_payload(raw, 3 * n, "colors").reshape(n, 3), want)


def test_colorize_point_cloud(pn2, cuda):
    import torch
    labels = np.random.RandomState(1).randint(0, 9, 5000)
    for dt in (torch.int32, torch.int64, torch.uint8):
        got = pn2.render.colorize_point_cloud(torch.from_numpy(labels).to(cuda).to(dt))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), np.array(pn2.render.LABEL_COLORS, dtype=np.uint8)[labels])
    for bad in (9, -1):
        labels[77] = bad
        for dt in (torch.int32, torch.int64):
            with pytest.raises(ValueError, match="outside"):
                pn2.render.colorize_point_cloud(torch.from_numpy(labels).to(cuda).to(dt))
    assert pn2.render.colorize_point_cloud(torch.zeros(0, dtype=torch.int32, device=cuda)).shape == (0, 3)


# ---- pn2.render ----------------------------------------------------------------------------------------------------------------
def _scene(n, seed=0):
    """a slab 40 x 25 x 6 m, x-sorted as the store keeps scenes, with labels by height"""
    rs = np.random.RandomState(seed)
    p = rs.uniform([-20.0, 5.0, -1.0], [20.0, 30.0, 5.0], (n, 3))
    p = p[np.argsort(p[:, 0], kind="stable")]
    return p, np.clip(((p[:, 2] + 1.0) * 1.5).astype(np.int32), 0, 8)


def _model_image(points, colors, view, w, h, size, perspective=False, background=(0, 0, 0)):
    z = R.empty(w, h)
    culled = R.splat(z, points, view, w, h, size, 0, perspective)
    return R.resolve(z, w, h, colors, background) + (culled,)


@pytest.mark.parametrize("view", ["top", "front", "side", "iso"])
def test_fit_view_puts_every_point_inside(pn2, cuda, view):
    import torch
    w, h, margin = 200, 120, 0.05
    pts, _ = _scene(2000, 3)
    d_pts = torch.from_numpy(pts).to(cuda)
    for perspective in (False, True):
        m = pn2.render.fit_view(d_pts, view, w, h, margin, perspective=perspective)
        assert isinstance(m, np.ndarray) and m.shape == (3, 4) and m.dtype == np.float64
        r = pn2.render.Renderer(w, h, 1, device=cuda)
        r.splat(d_pts, m, perspective=perspective)
        assert r.culled == 0
        u, v, d, ok = R.project(pts, m, perspective)
        assert ok.all() and (d >= 0).all()
        assert u.min() >= margin * w - 1e-6 and u.max() <= (1 - margin) * w + 1e-6
        assert v.min() >= margin * h - 1e-6 and v.max() <= (1 - margin) * h + 1e-6
        if not perspective:
            # aspect preserved: the tighter axis touches its margins (to rounding), the other is centred; depth starts at 0
            slack_u, slack_v = u.min() - margin * w, v.min() - margin * h
            assert min(slack_u, slack_v) < 1e-6 and abs(slack_u - ((1 - margin) * w - u.max())) < 1e-6 \
                and abs(slack_v - ((1 - margin) * h - v.max())) < 1e-6 and abs(d.min()) < 1e-9
            scale = np.linalg.norm(m[:2, :3], axis=1)
            assert abs(scale[0] - scale[1]) < 1e-9 * scale[0] and abs(m[0, :3] @ m[1, :3]) < 1e-9 * scale[0] ** 2
    # the image row grows downward and depth away from the viewer: the top view looks down on the scene, north up
    top = pn2.render.fit_view(d_pts, "top", w, h, margin)
    assert top[0, 0] > 0 and top[1, 1] < 0 and top[2, 2] < 0
    for name in ("front", "side", "iso"):
        assert pn2.render.fit_view(d_pts, name, w, h, margin)[1, 2] < 0  # up in the world is up in the image
    # margin 0 and a degenerate cloud (one point) still land inside
    for cloud in (d_pts, d_pts[:1], d_pts[:2]):
        r = pn2.render.Renderer(w, h, 1, device=cuda)
        r.splat(cloud, pn2.render.fit_view(cloud, view, w, h, 0.0))
        assert r.culled == 0


def test_renderer_equals_the_model(pn2, cuda):
    import torch
    w, h, n = 160, 90, 20000
    pts, labels = _scene(n)
    d_pts, d_lab = torch.from_numpy(pts).to(cuda), torch.from_numpy(labels).to(cuda)
    colors = np.array(pn2.render.LABEL_COLORS, dtype=np.uint8)[labels]
    view = pn2.render.fit_view(d_pts, "iso", w, h)
    r = pn2.render.Renderer(w, h, 2, (10, 20, 30), cuda)
    d_col = pn2.render.colorize_point_cloud(d_lab)
    for half in (slice(n // 2, n), slice(0, n // 2)):  # two chunks, the later one first
        r.splat(d_pts[half], view, half.start)
    want = _model_image(pts, colors, view, w, h, 2, background=(10, 20, 30))
    image, depth, index = r.image(d_col), r.depth(), r.indices()
    assert image.shape == (h, w, 3) and image.dtype == torch.uint8 and depth.dtype == torch.float32 and index.dtype == torch.int32
    assert np.array_equal(image.cpu().numpy(), want[0]) and depth.cpu().numpy().tobytes() == want[1].tobytes()
    assert np.array_equal(index.cpu().numpy(), want[2]) and r.culled == want[3] == 0
    assert (want[2] == -1).any() and (want[2] >= 0).any()
    buffers = [t.data_ptr() for t in (r._zbuf, r._image, r._depth, r._index)]
    # the one-call forms, float32 points; a reused renderer allocates nothing new
    p32 = d_pts.float()
    got = pn2.render.render_labels(p32, d_lab, "top", width=w, height=h, size=3, renderer=r)
    view = pn2.render.fit_view(p32, "top", w, h)
    want = _model_image(p32.cpu().numpy(), colors, view, w, h, 2, background=(10, 20, 30))  # the renderer's size and background win
    assert np.array_equal(got.cpu().numpy(), want[0]) and r.culled == 0
    assert buffers == [t.data_ptr() for t in (r._zbuf, r._image, r._depth, r._index)]
    got = pn2.render.render_colors(d_pts, d_col, "front", w, h, 1, (0, 0, 0), perspective=True)
    view = pn2.render.fit_view(d_pts, "front", w, h, perspective=True)
    assert np.array_equal(got.cpu().numpy(), _model_image(pts, colors, view, w, h, 1, True)[0])
    r.clear()
    assert r.culled == 0 and (r.indices() == -1).all() and torch.isinf(r.depth()).all()
    assert (r.image(d_col).cpu().numpy() == np.array([10, 20, 30], dtype=np.uint8)).all()


def test_renderer_captured_in_a_graph(pn2, cuda):
    """clear + splat + the three resolves as one graph, replayed on new point values: the eager result, and the model's"""
    import torch
    w, h, n = 96, 64, 5000
    clouds = [_scene(n, seed)[0].astype(np.float32) for seed in (1, 2, 3)]
    colors = np.random.RandomState(0).randint(0, 256, (n, 3)).astype(np.uint8)
    d_col = torch.from_numpy(colors).to(cuda)
    static = torch.from_numpy(clouds[0]).to(cuda)
    view = pn2.render.fit_view(static, "top", w, h)  # frozen into the capture
    r = pn2.render.Renderer(w, h, 2, device=cuda)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.clear()
        r.splat(static, view)
        image, depth, index = r.image(d_col), r.depth(), r.indices()
    for cloud in clouds[1:] + clouds[:1]:
        static.copy_(torch.from_numpy(cloud))
        g.replay()
        torch.cuda.synchronize()
        want = _model_image(cloud, colors, view, w, h, 2)
        assert np.array_equal(image.cpu().numpy(), want[0]) and depth.cpu().numpy().tobytes() == want[1].tobytes()
        assert np.array_equal(index.cpu().numpy(), want[2]) and r.culled == want[3]
        eager = pn2.render.Renderer(w, h, 2, device=cuda)
        eager.splat(static, view)
        assert torch.equal(eager.image(d_col), image) and torch.equal(eager.indices(), index) and eager.culled == r.culled


# ---- the examples --------------------------------------------------------------------------------------------------------------
def _read_png(path):
    import struct
    import zlib
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, data, shape = 8, b"", None
    while at < len(raw):
        length, kind = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + length]
        assert struct.unpack(">I", raw[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            shape = struct.unpack(">IIBBBBB", body)
        data += body if kind == b"IDAT" else b""
        at += 12 + length
    w, h = shape[:2]
    assert shape[2:] == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(data), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_examples_colorize_and_visualize(pn2, cuda, tmp_path):
    import torch
    n, w, h = 5000, 320, 200
    pts, labels = _scene(n, 4)
    truth = labels.copy()
    truth[::9] = (truth[::9] + 1) % 9
    file_colors = np.random.RandomState(2).randint(0, 256, (n, 3)).astype(np.uint8)
    scene, lab, gt = (str(tmp_path / name) for name in ("scene.pcd", "scene.labels", "truth.labels"))
    pn2.write_point_cloud_pcd(scene, torch.from_numpy(pts.astype(np.float32)).to(cuda), torch.from_numpy(file_colors).to(cuda))
    pn2.write_labels(lab, torch.from_numpy(labels).to(cuda))
    pn2.write_labels(gt, torch.from_numpy(truth).to(cuda))
    table = np.array(pn2.render.LABEL_COLORS, dtype=np.uint8)

    def run(script, *args):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)] + [str(a) for a in args], cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, p.stdout.decode(errors="replace")

    out = str(tmp_path / "colored.ply")
    run("colorize.py", scene, lab, out)
    got_pts, got_col = pn2.read_point_cloud(out, cuda)
    assert np.array_equal(got_pts.cpu().numpy(), pts.astype(np.float32).astype(np.float64))
    assert np.array_equal(np.floor(got_col.cpu().numpy() * 255.0).astype(np.uint8), table[labels])  # the table's bytes
    os.makedirs(str(tmp_path / "pd"))
    for name in ("a", "b"):
        pn2.write_point_cloud_pcd(str(tmp_path / "pd" / (name + ".pcd")), torch.from_numpy(pts).to(cuda))
        pn2.write_labels(str(tmp_path / "pd" / (name + ".labels")), torch.from_numpy(labels if name == "a" else truth).to(cuda))
    run("colorize.py", "--pd_dir", "pd")  # the directory form of the reference's __main__
    for name, want in (("a", labels), ("b", truth)):
        got_pts, got_col = pn2.read_point_cloud(str(tmp_path / "pd_colorized" / (name + ".pcd")), cuda)
        assert np.array_equal(got_pts.cpu().numpy(), pts.astype(np.float32).astype(np.float64))
        assert np.array_equal(np.floor(got_col.cpu().numpy() * 255.0).astype(np.uint8), table[want])

    p32 = torch.from_numpy(pts.astype(np.float32).astype(np.float64)).to(cuda)  # what the reader returns
    cases = [((), file_colors, "top", 2, False),
             (("--labels_path", lab, "--compare", gt, "--view", "iso", "--size", 3, "--perspective"),
              np.where((labels != truth)[:, None], np.array([255, 0, 0], dtype=np.uint8), table[labels]), "iso", 3, True)]
    for k, (args, colors, view, size, perspective) in enumerate(cases):
        out = str(tmp_path / ("view%d.png" % k))
        run("visualize.py", "--pcd_path", scene, "--out", out, "--width", w, "--height", h, *args)
        want = pn2.render.render_colors(p32, torch.from_numpy(np.ascontiguousarray(colors)).to(cuda), view, w, h, size,
                                        perspective=perspective)
        got = _read_png(out)
        assert np.array_equal(got, want.cpu().numpy()) and (got != 0).any()
