"""tools/sa_row_packing_stats.py: the CPU count of what the packed SA kernels skip -- classifier and tile count on hand-made rows"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("sa_row_packing_stats", os.path.join(ROOT, "tools", "sa_row_packing_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classifier_reads_the_live_prefix_not_the_distinct_count():
    t = _tool()
    rows = np.full((5, 32), 5, dtype=np.int32)
    rows[1, 7] = 9    # live 8
    rows[2, 8] = 9    # live 9
    rows[3, 20] = 7   # two distinct values, but the odd one sits late: class 32
    rows[4, :] = 0    # an empty ball
    assert list(t.live_slots(rows)) == [1, 8, 9, 21, 1]
    assert list(t.classes(rows)) == [8, 8, 16, 32, 8]


def test_tile_count_of_a_block():
    t = _tool()
    assert t.packed_tiles(np.array([8] * 8), 64) == 2
    assert t.packed_tiles(np.array([8] * 9), 64) == 3
    assert t.packed_tiles(np.array([16, 16, 16]), 64) == 2
    assert t.packed_tiles(np.array([32, 16, 8]), 64) == 2      # the class-8 group rides with the odd class-16 one
    assert t.packed_tiles(np.array([16] + [8] * 5), 64) == 2   # 5 = 4 + 1: the fifth rides along
    assert t.packed_tiles(np.array([16] + [8] * 6), 64) == 3   # 6 = 4 + 2: nothing saved by moving one
    assert t.packed_tiles(np.array([8] * 8), 4) == 2
    assert t.packed_tiles(np.array([32] * 7), 64) == 7
