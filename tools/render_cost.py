"""What a rendered frame costs ("Rendering"): one JSON line with, in this one process, the medians of 7
rounds, the device synchronised on both sides of each region, the two forms alternating within a round:
  hip     pn2.render.Renderer: clear (a 0xFF fill) + pn2_render_splat + pn2_render_resolve to the RGB image, and the three steps
          alone;
  torch   the same steps restated in torch ops: the projection in float64 in the kernel's association, the keys in int64 (the
          ordered depth word moved by 2^31 so that the signed order is the unsigned one), one scatter_reduce_(..., "amin") per
          pixel of the splat, and a gather of the colours -- checked to give the renderer's z-buffer and image first.
The frame is 1920 x 1080; the cloud a 200 m x 110 m x 30 m slab of 4 * 10^6 and 10^7 float32 points sorted by x, as the scene
store keeps them, seen from above (fit_view "top"), at size 1 and 3.
With --ab-library the splat of a second build of the library is timed in the same rounds, into the same emptied buffer, after
its z-buffer has been checked to be the same: the build with -DPN2_RENDER_ALWAYS_ATOMIC sends every pixel visit as an atomic,
without the plain load in front of it.
usage: python tools/render_cost.py [--points 4000000 10000000] [--sizes 1 3] [--rounds 7] [--ab-library PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pn2_amd as pn2  # noqa: E402

W, H = 1920, 1080
SIGN = -(1 << 63)


def scene(n, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    p = torch.rand((n, 3), generator=g, device=dev, dtype=torch.float32) * torch.tensor([200.0, 110.0, 30.0], device=dev)
    p = p[torch.argsort(p[:, 0])].contiguous()
    colors = torch.randint(0, 256, (n, 3), generator=g, device=dev, dtype=torch.uint8)
    return p, colors


class TorchRenderer:
    """clear / splat / image in torch ops; zbuf has one slot more than the image: where the pixels outside it are sent"""

    def __init__(self, size, dev):
        self.size, self.dev = size, dev
        self.zbuf = torch.empty((H * W + 1,), dtype=torch.int64, device=dev)
        self.bg = torch.zeros((3,), dtype=torch.uint8, device=dev)

    def clear(self):
        self.zbuf.fill_(2 ** 63 - 1)

    def splat(self, points, view):
        m = [[float(v) for v in row] for row in view]
        x, y, z = (points[:, c].double() for c in range(3))
        u, v, d = (((r[0] * x + r[1] * y) + r[2] * z) + r[3] for r in m)
        ok = (u >= -2.0 ** 30) & (u < 2.0 ** 30) & (v >= -2.0 ** 30) & (v < 2.0 ** 30) & torch.isfinite(d)
        px = torch.where(ok, u, 0.0).floor().long()
        py = torch.where(ok, v, 0.0).floor().long()
        bits = (d.float() + 0.0).view(torch.int32).long() & 0xFFFFFFFF
        k = torch.where(bits >= 2 ** 31, 0xFFFFFFFF - bits, bits + 2 ** 31)
        key = ((k - 2 ** 31) << 32) | torch.arange(points.shape[0], device=self.dev)
        for b in range(self.size):
            for a in range(self.size):
                qx, qy = px - self.size // 2 + a, py - self.size // 2 + b
                inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                self.zbuf.scatter_reduce_(0, torch.where(inside, qy * W + qx, H * W), key, "amin")

    def image(self, colors):
        key = self.zbuf[:H * W]
        index = key & 0xFFFFFFFF
        has = (key != 2 ** 63 - 1) & (index < colors.shape[0])
        return torch.where(has[:, None], colors[torch.where(has, index, 0)], self.bg).reshape(H, W, 3)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(runs):
    return {"median_ms": round(float(np.median(runs)), 3), "runs_ms": [round(r, 3) for r in runs]}


def variant_splat(path):
    """pn2_render_splat of another build of the library (--ab-library), bound from the same header"""
    import ctypes
    fn = ctypes.CDLL(path).pn2_render_splat
    sig = pn2._lib.ABI.functions["pn2_render_splat"]
    fn.argtypes, fn.restype = sig.argtypes, sig.restype
    return fn


def case(n, size, rounds, dev, ab=None):
    points, colors = scene(n, dev)
    view = pn2.render.fit_view(points, "top", W, H)
    hip, ref = pn2.render.Renderer(W, H, size, device=dev), TorchRenderer(size, dev)
    m = pn2.render._view_array(view)

    def ab_splat():  # the variant's splat into the renderer's own buffers
        pn2._lib.check(ab(n, 0, pn2._lib.ptr(points), 0, m, 0, W, H, size, pn2._lib.ptr(hip._zbuf), pn2._lib.ptr(hip._culled),
                          pn2._lib.stream_ptr()), "the variant's pn2_render_splat")

    def hip_frame():
        hip.clear()
        hip.splat(points, view)
        return hip.image(colors)

    def torch_frame():
        ref.clear()
        ref.splat(points, view)
        return ref.image(colors)

    a, b = hip_frame(), torch_frame()  # also the warm-up of every shape timed below
    if not torch.equal(hip._zbuf ^ SIGN, ref.zbuf[:H * W]) or not torch.equal(a, b):
        raise SystemExit("the torch restatement disagrees with the renderer at n=%d size=%d" % (n, size))
    covered = int((hip.indices() >= 0).sum())
    if ab is not None:
        hip.clear()
        ab_splat()
        if not torch.equal(hip._zbuf ^ SIGN, ref.zbuf[:H * W]):
            raise SystemExit("the variant's splat disagrees at n=%d size=%d" % (n, size))
    steps = {"clear": hip.clear, "splat": lambda: hip.splat(points, view), "resolve": lambda: hip.image(colors)}
    t = {"hip": [], "torch": [], "clear": [], "splat": [], "resolve": []}
    if ab is not None:
        t["splat_variant"] = []
    for _ in range(rounds):
        t["hip"].append(wall_ms(hip_frame))
        t["torch"].append(wall_ms(torch_frame))
        for name in ("clear", "splat", "resolve"):  # in frame order: the splat meets an empty buffer, as in a frame
            t[name].append(wall_ms(steps[name]))
        if ab is not None:
            hip.clear()
            t["splat_variant"].append(wall_ms(ab_splat))
    out = {"points": n, "size": size, "pixels_covered": covered, "culled": hip.culled}
    out.update({name: summary(runs) for name, runs in t.items()})
    out["torch_over_hip"] = round(out["torch"]["median_ms"] / out["hip"]["median_ms"], 2)
    out["splat_points_per_us"] = round(n / (out["splat"]["median_ms"] * 1e3), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[4000000, 10000000])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ab-library", default="", help="another build of libpn2_hip.so: its pn2_render_splat is timed beside the "
                    "shipped one (build.build(extra_flags=['-DPN2_RENDER_ALWAYS_ATOMIC'], out=...): no load before the atomic)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ab = variant_splat(args.ab_library) if args.ab_library else None
    out = {"width": W, "height": H, "ab_library": os.path.basename(args.ab_library),
           "cases": [case(n, s, args.rounds, dev, ab) for n in args.points for s in args.sizes]}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
