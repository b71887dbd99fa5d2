"""tools/sa_row_packing_stats.py, chunk_tiles: the CPU restatement of the wide kernel's chunk packer (csrc/pn2_mlp_wide.hip, PACK).
Its invariants on random and hand-made class lists: every group sits in exactly one slot, a slot is at least as large as the
group's class, and the tile count is the formula the kernel's workgroups return by."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("sa_row_packing_stats", os.path.join(ROOT, "tools", "sa_row_packing_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases():
    rs = np.random.RandomState(0)
    out = [np.array([8]), np.array([16]), np.array([32]), np.array([16] + [8] * 5), np.array([16] + [8] * 6),
           np.array([8] * 7), np.array([32, 16, 8]), np.array([16, 16, 16, 8]), np.full(256, 8), np.full(256, 32)]
    for n in (1, 7, 44, 100, 255, 256):
        for p in ((0.6, 0.3, 0.1), (0.1, 0.1, 0.8), (0.34, 0.33, 0.33)):
            out.append(rs.choice([8, 16, 32], size=n, p=p))
    return out


@pytest.mark.parametrize("cls", _cases(), ids=lambda c: "n%d_%d" % (len(c), int(c.sum())))
def test_chunk_tiles_invariants(cls):
    t = _tool()
    base = 512
    tiles = t.chunk_tiles(cls, base)
    seen = [g for _, gs in tiles for g in gs]
    assert sorted(seen) == list(range(base, base + len(cls)))          # every group exactly once
    for s, gs in tiles:
        assert s in (8, 16, 32) and 1 <= len(gs) <= 32 // s
        assert all(s >= cls[g - base] for g in gs)                      # slot size >= live slots (through the class)
    assert [s for s, _ in tiles] == sorted((s for s, _ in tiles), reverse=True)  # class-32 tiles, then 16, then 8
    assert len(tiles) == t.packed_tiles(cls, t.WIDE_CHUNK)              # the formula
    assert len(tiles) <= len(cls)                                       # never more workgroups than the grid has


def test_take_along_rule_moves_the_last_class8_group():
    t = _tool()
    tiles = t.chunk_tiles(np.array([8, 16, 8, 8, 8, 8]), 0)            # one class 16, 4k + 1 class 8
    assert tiles == [(16, [1, 5]), (8, [0, 2, 3, 4])]
    tiles = t.chunk_tiles(np.array([8, 16, 8, 8, 8, 8, 8]), 0)         # 4k + 2: nothing saved, nothing moved
    assert tiles == [(16, [1]), (8, [0, 2, 3, 4]), (8, [5, 6])]
