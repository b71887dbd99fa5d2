#!/usr/bin/env python
"""The premise of the SA row packing (csrc/pn2_sa_fused.hip, PACK), counted on the CPU: for a benchmark input, how many of the
32 rows of a ball-query group are live, and how many 32-row tiles the packed kernels run per tile of the un-packed ones.

    python tools/sa_row_packing_stats.py [--input s_scene|s_randn|s_dup25] [--clouds 16] [--points 8192] [--block 64] [--wide]

Geometry from the CPU oracle (oracle/), inputs from benchlib.inputs (seed 0), levels from SEMANTIC_HYPERPARAMS.  A group's
class is the smallest s in {8, 16, 32} with idx[j] == idx[0] for all j >= s; a block of `--block` consecutive centres packs
four class-8 or two class-16 groups into a tile (an odd class-16 group takes one class-8 group along when that saves a tile),
exactly as the kernel does.  --wide: the wide kernel's packer (csrc/pn2_mlp_wide.hip, PACK) -- chunks of 256 consecutive groups,
one workgroup per tile of the chunk's list (chunk_tiles below restates it); the count is then that of --block 256.  No GPU needed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEVELS = ((1024, 0.5), (256, 1.0), (64, 2.0), (16, 4.0))  # npoint, radius of SA1..SA4 (model.SEMANTIC_HYPERPARAMS), nsample 32


def live_slots(idx):
    """(..., 32) index rows -> 1 + the last position that differs from position 0"""
    diff = idx != idx[..., :1]
    last = idx.shape[-1] - 1 - np.argmax(diff[..., ::-1], axis=-1)
    return np.where(diff.any(axis=-1), last + 1, 1)


def classes(idx):
    live = live_slots(idx).reshape(-1)
    return np.where(live <= 8, 8, np.where(live <= 16, 16, 32))


def packed_tiles(cls, block):
    """tiles the kernel runs for the groups `cls` (flat, in order) taken in blocks of `block`"""
    tiles = 0
    for lo in range(0, len(cls), block):
        c = cls[lo:lo + block]
        n32, n16, n8 = int((c == 32).sum()), int((c == 16).sum()), int((c == 8).sum())
        if (n16 & 1) and (n8 & 3) == 1:
            n16, n8 = n16 + 1, n8 - 1
        tiles += n32 + (n16 + 1) // 2 + (n8 + 3) // 4
    return tiles


WIDE_CHUNK = 256  # groups per chunk of the wide kernel's packer = threads of a workgroup


def chunk_tiles(cls, base=0):
    """The wide kernel's tile list of ONE chunk: cls = classes of its (at most WIDE_CHUNK) consecutive groups, base = id of the
    first.  -> [(slot rows, [group ids, one per filled slot])]: class-32 tiles, then pairs of class 16, then fours of class 8, the
    groups of a class in their own order; an odd class-16 group takes the LAST class-8 group along when that saves a tile.
    Workgroup j of the chunk runs tile j; the workgroups behind the list return."""
    cls = np.asarray(cls)
    assert 0 < len(cls) <= WIDE_CHUNK
    g32 = [base + i for i in np.flatnonzero(cls == 32)]
    g16 = [base + i for i in np.flatnonzero(cls == 16)]
    g8 = [base + i for i in np.flatnonzero(cls == 8)]
    if (len(g16) & 1) and (len(g8) & 3) == 1:
        g16.append(g8.pop())
    tiles = [(32, [g]) for g in g32]
    tiles += [(16, g16[i:i + 2]) for i in range(0, len(g16), 2)]
    tiles += [(8, g8[i:i + 4]) for i in range(0, len(g8), 4)]
    return tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="s_scene", choices=("s_scene", "s_randn", "s_dup25"))
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--wide", action="store_true", help="the wide kernel's packer: chunks of %d groups" % WIDE_CHUNK)
    args = ap.parse_args()
    if args.wide and args.block != ap.get_default("block"):
        ap.error("--wide fixes the chunk at %d groups: do not give --block with it" % WIDE_CHUNK)
    from benchlib import inputs
    from oracle import oracle as O
    O.build()
    xyz = np.ascontiguousarray(getattr(inputs, args.input)(0, args.clouds, args.points)[:, :, :3])
    print("%-8s %-5s %7s %14s   %-22s %s" % ("input", "level", "groups", "live rows/32", "class 8 / 16 / 32", "tile ratio"))
    for lv, (npoint, radius) in enumerate(LEVELS, 1):
        new_xyz = O.gather_point(xyz, O.farthest_point_sample(npoint, xyz))
        idx, _ = O.query_ball_point(radius, 32, xyz, new_xyz)
        idx = np.asarray(idx).reshape(-1, 32)
        cls = classes(idx)
        print("%-8s SA%d   %7d %14.1f   %.2f / %.2f / %.2f     %.2f" % (
            args.input, lv, len(cls), live_slots(idx).mean(), (cls == 8).mean(), (cls == 16).mean(), (cls == 32).mean(),
            (sum(len(chunk_tiles(cls[lo:lo + WIDE_CHUNK], lo)) for lo in range(0, len(cls), WIDE_CHUNK)) if args.wide
             else packed_tiles(cls, args.block)) / float(len(cls))))
        xyz = new_xyz


if __name__ == "__main__":
    main()
