"""CPU tests around the tiled cover of a scene (csrc/pn2_tile.hip, predict.predict_scene_tiled): the numpy model of the rule
(tests/tile_ref.py) on cases worked out by hand, its invariant on random scenes, the header's prototypes and the refusals of
the four entry points.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tile_ref as M  # noqa: E402


def _line(xs, y=0.0, z=0.0):
    """points on a line of constant y and z at the given (ascending) x"""
    return np.array([[x, y, z] for x in xs], dtype=np.float64)


def _rows(pl, npts):
    return [M.sample_rows(pl, q, npts)[0].tolist() for q in range(len(pl["samples"]))]


def test_a_single_point():
    """n = 1, N = 4: one tile (0, 0), a = 0, m = 1, S = 1, c = 1; all four rows are point 0, the first one live.
    The point (3, 4, 5) with box 10: box_min is the point, shift = (3 + 5, 4 + 5, 5), so every row is (-5, -5, 0)."""
    p = np.array([[3.0, 4.0, 5.0]])
    pl = M.plan(p, 10, 10, 4)
    assert pl["order"].tolist() == [0] and pl["samples"].tolist() == [[0, 1, 0, 1]] and pl["header"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert pl["order"].dtype == np.int32 and pl["samples"].dtype == np.int32 and pl["header"].dtype == np.int32
    col = np.array([[0.25, 0.5, 0.75]], dtype=np.float32)
    data, sel, live = M.batch(pl, p, col, 0, 2, 4, 10, 10)
    assert data.dtype == np.float32 and data.shape == (2, 4, 6) and sel.dtype == np.int32 and live.dtype == np.int32
    assert sel.tolist() == [[0] * 4] * 2 and live.tolist() == [1, 0]  # slot 1 lies beyond the table: a copy that does not vote
    assert (data[:, :, :3] == [-5.0, -5.0, 0.0]).all() and (data[:, :, 3:] == col[0]).all()
    data, sel, live = M.batch(pl, p, None, 1, 1, 4, 10, 10)  # wholly beyond
    assert data.shape == (1, 4, 3) and live.tolist() == [0] and sel.tolist() == [[0] * 4]


def test_tiles_of_n_n_plus_one_and_two_n_points():
    """N = 4, every point in tile (0, 0) (x in [0, 10)), so order is the identity.
    m = 4: S = 1, c = 4, rows 0 1 2 3.
    m = 5: S = 2; sample 0 owns ranks 0 2 4 (c = 3), rows 0 2 4 0; sample 1 owns ranks 1 3 (c = 2), rows 1 3 1 3.
    m = 8: S = 2, c = 4 twice: rows 0 2 4 6 and 1 3 5 7."""
    pl = M.plan(_line([0, 1, 2, 3]), 10, 10, 4)
    assert pl["samples"].tolist() == [[0, 4, 0, 1]] and _rows(pl, 4) == [[0, 1, 2, 3]]
    pl = M.plan(_line([0, 1, 2, 3, 4]), 10, 10, 4)
    assert pl["samples"].tolist() == [[0, 5, 0, 2], [0, 5, 1, 2]] and _rows(pl, 4) == [[0, 2, 4, 0], [1, 3, 1, 3]]
    assert [M.sample_rows(pl, q, 4)[1] for q in range(2)] == [3, 2]
    pl = M.plan(_line(range(8)), 10, 10, 4)
    assert pl["samples"].tolist() == [[0, 8, 0, 2], [0, 8, 1, 2]] and _rows(pl, 4) == [[0, 2, 4, 6], [1, 3, 5, 7]]
    assert pl["header"].tolist()[:4] == [1, 2, 0, 0]


def test_the_ragged_last_samples():
    """m = 10, N = 4: S = 3; c = ceil(10 / 3), ceil(9 / 3), ceil(8 / 3) = 4, 3, 3: rows 0 3 6 9 | 1 4 7 1 | 2 5 8 2"""
    pl = M.plan(_line(np.arange(10) * 0.5), 10, 10, 4)
    assert pl["samples"].tolist() == [[0, 10, s, 3] for s in range(3)]
    assert _rows(pl, 4) == [[0, 3, 6, 9], [1, 4, 7, 1], [2, 5, 8, 2]]
    assert [M.sample_rows(pl, q, 4)[1] for q in range(3)] == [4, 3, 3]


def test_a_point_on_a_boundary_belongs_to_the_upper_tile():
    """x = 0, 10, 20 with box 10 and ox = 0: i = 0, 1, 2 (10 / 10 = 1 exactly).  y = 0, 8, 4 with box 4, oy = 0: j = 0, 2, 1.
    Three tiles of one point; with phase (10, 4) every index grows by exactly one and the tiles stay the same."""
    p = np.array([[0.0, 0.0, 0.0], [10.0, 8.0, 0.0], [20.0, 4.0, 0.0]])
    for ph in ((0.0, 0.0), (10.0, 4.0)):
        pl = M.plan(p, 10, 4, 4, ph)
        assert pl["order"].tolist() == [0, 1, 2] and pl["samples"].tolist() == [[0, 1, 0, 1], [1, 1, 0, 1], [2, 1, 0, 1]]
    # the same x pair one ulp below the boundary shares tile 0: the model floors a quotient, it does not compare with 10
    q = _line([0.0, np.nextafter(10.0, 0.0)])
    assert M.plan(q, 10, 10, 4)["samples"].tolist() == [[0, 2, 0, 1]]
    # y decides inside one x column: (0, 0) (0, 1) -> order by j
    r = np.array([[0.0, 4.0, 0.0], [1.0, 0.0, 0.0], [2.0, 3.999, 0.0]])
    assert M.plan(r, 10, 4, 4)["order"].tolist() == [1, 2, 0]


def test_negative_coordinates():
    """x = -25, -15.5, -5; y = -3, -13, -8; box 10: ox = -25, oy = -13.  i = floor(0), floor(0.95), floor(2) = 0, 0, 2;
    j = floor(1), floor(0), floor(0.5) = 1, 0, 0.  Keys (0,1) (0,0) (2,0): order 1 0 2, three tiles.
    With phase (5, 5): ox = -30, oy = -18: i = 0, 1, 2; j = 1, 0, 1: order 0 1 2."""
    p = np.array([[-25.0, -3.0, 1.0], [-15.5, -13.0, 2.0], [-5.0, -8.0, 3.0]])
    pl = M.plan(p, 10, 10, 2)
    assert pl["order"].tolist() == [1, 0, 2] and pl["samples"].tolist() == [[0, 1, 0, 1], [1, 1, 0, 1], [2, 1, 0, 1]]
    assert pl["header"].tolist()[:4] == [3, 3, 0, 0]
    assert M.plan(p, 10, 10, 2, (5.0, 5.0))["order"].tolist() == [0, 1, 2]
    # sample 0 is point 1 alone: shift = (-15.5 + 5, -13 + 5, 2) -> (-5, -5, 0)
    data, sel, live = M.batch(pl, p, None, 0, 3, 2, 10, 10)
    assert sel.tolist() == [[1, 1], [0, 0], [2, 2]] and live.tolist() == [1, 1, 1] and (data == [-5.0, -5.0, 0.0]).all()


def test_min_points_skips_a_known_tile():
    """x = 0, 1, 2 in tile 0 and x = 15 in tile 1; min_points = 2 skips the second: 2 tiles, 1 sample, 1 skipped point.
    min_points = 4 skips both: no sample, 4 skipped, and a batch of zeros with sel = -1."""
    p = _line([0, 1, 2, 15])
    pl = M.plan(p, 10, 10, 4, min_points=2)
    assert pl["header"].tolist()[:4] == [2, 1, 1, 0] and pl["samples"].tolist() == [[0, 3, 0, 1]]
    pl = M.plan(p, 10, 10, 4, min_points=4)
    assert pl["header"].tolist()[:4] == [2, 0, 4, 0] and pl["samples"].shape == (0, 4)
    data, sel, live = M.batch(pl, p, None, 0, 2, 4, 10, 10)
    assert not data.any() and (sel == -1).all() and live.tolist() == [0, 0]


def test_statuses():
    p = _line([0, 1, 2, 15])
    q = p.copy()
    q[2, 1] = np.nan
    assert M.plan(q, 10, 10, 4)["header"][3] == 1
    q[2, 1] = np.inf
    assert M.plan(q, 10, 10, 4)["header"][3] == 1
    q = p.copy()
    q[2, 2] = np.nan  # z takes no part in the grid
    assert M.plan(q, 10, 10, 4)["header"][3] == 0
    assert M.plan(_line([0.0, 1.0]), 2.0 ** -31, 10, 4)["header"][3] == 2  # i = 2^31
    assert M.plan(_line([0.0, 1.0]), 2.0 ** -30, 10, 4)["header"][3] == 0  # i = 2^30
    pl = M.plan(_line(np.arange(10) * 0.5), 10, 10, 4, sample_cap=2)
    assert pl["header"].tolist()[:4] == [1, 3, 0, 3] and pl["samples"].tolist() == [[0, 10, 0, 3], [0, 10, 1, 3]]


def test_the_y_minimum_among_zeros_is_the_negative_one():
    p = np.array([[0.0, 0.0, 0.0], [1.0, -0.0, 0.0], [2.0, 3.0, -0.0]])
    assert np.signbit(M._min_signed(p[:, 1])) and not np.signbit(M._min_signed(p[:, 0])) and np.signbit(M._min_signed(p[:, 2]))
    # z - (-0.0): the row whose z is -0.0 comes out as +0.0, the others as +0.0 too
    data, _, _ = M.batch(M.plan(p, 10, 10, 4), p, None, 0, 1, 4, 10, 10)
    assert not np.signbit(data[0, :, 2]).any()


def test_vote_and_labels_by_hand():
    """three points, C = 3.  Batch of 2 samples of 3 rows: sample 0 live 2 (rows 0, 1 -> points 0, 1), sample 1 live 3.
    Predictions 2, 1, (ignored) | 2, 7, -1: point 0 gets class 2 twice, point 1 class 1 once, two live rows are dropped.
    Labels: point 0 -> 2, point 1 -> 1, point 2 (no vote) -> 0; a tie 1:1 between classes 0 and 2 resolves to 0."""
    votes = np.zeros((3, 3), dtype=np.int32)
    sel = np.array([[0, 1, 0], [0, 1, 2]], dtype=np.int32)
    dropped = M.vote(votes, sel, np.array([2, 3], dtype=np.int32), np.array([[2, 1, 1], [2, 7, -1]], dtype=np.int32))
    assert dropped == 2 and votes.tolist() == [[0, 0, 2], [0, 1, 0], [0, 0, 0]]
    assert M.labels(votes).tolist() == [2, 1, 0] and M.labels(votes).dtype == np.int32
    assert M.labels(np.array([[1, 0, 1], [0, 3, 3]], dtype=np.int32)).tolist() == [0, 1]


@pytest.mark.parametrize("npts", [4, 64, 2048])
def test_every_point_is_live_exactly_once_per_pass(npts):
    """min_points = 1: over all samples of a pass, the live rows are a permutation of the scene; and no sample has more than
    npts live rows, so none is cut.  Uniform points in 25 m x 15 m, boxes of 10 m."""
    for n in (1, 63, 64, 65, 257, 4097, 20000):
        rs = np.random.RandomState(n)
        p = np.stack([np.sort(rs.uniform(0, 25, n)), rs.uniform(0, 15, n), rs.uniform(0, 3, n)], 1)
        for ph in ((0.0, 0.0), (5.0, 5.0), (2.5, 7.5)):
            pl = M.plan(p, 10, 10, npts, ph)
            assert pl["header"][3] == 0 and pl["header"][2] == 0
            assert np.array_equal(np.sort(pl["order"]), np.arange(n))
            S = pl["samples"]
            assert pl["header"][1] == len(S) <= n // npts + pl["header"][0] and pl["header"][0] <= 12
            seen = np.zeros(n, dtype=np.int64)
            for q in range(len(S)):
                a, m, s, k = (int(v) for v in S[q])
                c = -(-(m - s) // k)
                assert 1 <= c <= npts
                seen[pl["order"][a + s + np.arange(c) * k]] += 1
            assert (seen == 1).all(), (n, npts, ph)


def test_model_predict_scene_votes_once_per_phase():
    rs = np.random.RandomState(3)
    n = 500
    p = np.stack([np.sort(rs.uniform(0, 25, n)), rs.uniform(0, 15, n), rs.uniform(0, 3, n)], 1)
    predict = lambda data: (np.floor(data[:, :, 0] + 5.0).astype(np.int64) % 5)  # noqa: E731  (a function of the centred x)
    lab, votes = M.predict_scene(p, None, 10, 10, 16, 5, predict, 3, phases=((0, 0), (5, 5)))
    assert (votes.sum(1) == 2).all() and lab.shape == (n,) and np.array_equal(lab, np.argmax(votes, 1))


# ---- the header and the refusals ---------------------------------------------------------------------------------------------
ARGS = {
    "pn2_tile_plan_workspace_size": ("n", "bytes"),
    "pn2_tile_plan": ("n", "points", "box_size_x", "box_size_y", "phase_x", "phase_y", "npts", "min_points", "sample_cap", "order",
                      "samples", "header", "workspace", "workspace_bytes", "stream"),
    "pn2_tile_gather": ("b", "npts", "q0", "use_color", "points", "colors", "order", "samples", "header", "box_size_x",
                        "box_size_y", "out_data", "out_sel", "out_live", "stream"),
    "pn2_tile_vote": ("b", "npts", "num_class", "sel", "live", "pred", "votes", "dropped", "stream"),
    "pn2_tile_labels": ("n", "num_class", "votes", "labels", "stream"),
}


def test_header_declares_the_entry_points(pn2):
    fns = pn2._lib.ABI.functions
    for name, args in ARGS.items():
        assert fns[name].restype is ctypes.c_int and fns[name].argnames == args, name
        assert name in pn2._lib.SIGNATURES and name not in pn2._lib._TRACE_ARGS
        assert not any(a in ("nlayers", "widths", "running_mean") or a.startswith("ld") for a in args), name
        assert args[-1] == "stream" or name.endswith("_size")
    i, p, d, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_size_t
    assert fns["pn2_tile_plan"].argtypes == [i, p, d, d, d, d, i, i, i, p, p, p, p, z, p]
    assert fns["pn2_tile_gather"].argtypes == [i, i, i, i, p, p, p, p, p, d, d, p, p, p, p]
    assert "pn2_tile_vote" in pn2._lib._STATEFUL  # it adds into the caller's votes: never launched twice by the dup hook
    assert not {"pn2_tile_plan", "pn2_tile_gather", "pn2_tile_labels"} & pn2._lib._STATEFUL
    assert pn2._lib.ABI.constants["PN2_ABI_VERSION"] == 2


def _caller(pn2, name, good):
    names = pn2._lib.ABI.functions[name].argnames

    def call(**change):
        a = dict(good, **change)
        return getattr(pn2._lib.lib, name)(*[a[k] for k in names])
    return call


def test_argument_errors_are_refused_without_a_gpu(pn2):
    K = pn2._lib.ABI.constants
    EINVAL, ENULL, ERANGE, EUNSUP = K["PN2_EINVAL"], K["PN2_ENULL"], K["PN2_ERANGE"], K["PN2_EUNSUP"]
    MAXR = K["PN2_FRAME_MAX_ROWS"]
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before a launch
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)  # noqa: E731
    nan, inf = float("nan"), float("inf")

    plan = _caller(pn2, "pn2_tile_plan", dict(n=1000, points=fake, box_size_x=10.0, box_size_y=10.0, phase_x=0.0, phase_y=5.0,
                                             npts=64, min_points=1, sample_cap=1000, order=fake, samples=fake, header=fake,
                                             workspace=fake, workspace_bytes=0, stream=None))
    assert plan() == EINVAL                                   # the workspace is too small
    assert plan(workspace_bytes=4096) == EINVAL               # (less than the keys alone: no device is asked anything)
    for bad in (dict(n=0), dict(n=-3), dict(npts=0), dict(min_points=0), dict(sample_cap=-1), dict(box_size_x=0.0),
                dict(box_size_y=-1.0), dict(box_size_x=nan), dict(box_size_y=inf), dict(phase_x=-0.5), dict(phase_y=nan),
                dict(phase_x=inf)):
        assert plan(workspace_bytes=1 << 40, **bad) == EINVAL, bad
    assert plan(n=MAXR + 1) == ERANGE and plan(npts=MAXR + 1) == ERANGE
    assert plan(n=0, points=None) == EINVAL                   # the sizes are looked at first
    for required in ("points", "order", "samples", "header", "workspace"):
        assert plan(**{required: None}) == ENULL, required
    assert plan(samples=None, sample_cap=0) == EINVAL         # counting only: fine up to the workspace
    for name, k in (("points", 4), ("order", 2), ("samples", 8), ("header", 1), ("workspace", 128)):
        assert plan(workspace_bytes=1 << 40, **{name: odd(k)}) == EINVAL, name
    nbytes = ctypes.c_uint64(0)
    size = pn2._lib.lib.pn2_tile_plan_workspace_size
    assert size(0, ctypes.byref(nbytes)) == EINVAL and size(100, None) == ENULL and size(MAXR + 1, ctypes.byref(nbytes)) == ERANGE

    gather = _caller(pn2, "pn2_tile_gather", dict(b=4, npts=64, q0=0, use_color=1, points=fake, colors=fake, order=fake,
                                                 samples=fake, header=fake, box_size_x=10.0, box_size_y=10.0, out_data=fake,
                                                 out_sel=fake, out_live=fake, stream=None))
    for bad in (dict(b=0), dict(npts=0), dict(q0=-1), dict(box_size_x=0.0), dict(box_size_y=nan)):
        assert gather(**bad) == EINVAL, bad
    assert gather(npts=MAXR + 1) == ERANGE and gather(b=65536) == ERANGE and gather(b=40000, npts=1 << 16) == ERANGE
    for required in ("points", "colors", "order", "samples", "header", "out_data", "out_sel", "out_live"):
        assert gather(**{required: None}) == ENULL, required
    for name, k in (("points", 4), ("colors", 2), ("order", 1), ("samples", 4), ("header", 2), ("out_data", 2), ("out_sel", 1),
                    ("out_live", 3)):
        assert gather(**{name: odd(k)}) == EINVAL, name
    assert gather(b=0, points=None) == EINVAL

    vote = _caller(pn2, "pn2_tile_vote", dict(b=4, npts=64, num_class=9, sel=fake, live=fake, pred=fake, votes=fake, dropped=fake,
                                             stream=None))
    for bad in (dict(b=0), dict(npts=-1), dict(num_class=0)):
        assert vote(**bad) == EINVAL, bad
    assert vote(num_class=65) == EUNSUP and vote(b=1 << 16, npts=1 << 16) == ERANGE
    for required in ("sel", "live", "pred", "votes"):
        assert vote(**{required: None}) == ENULL, required
    for name, k in (("sel", 1), ("live", 2), ("pred", 3), ("votes", 2), ("dropped", 4)):
        assert vote(**{name: odd(k)}) == EINVAL, name

    labels = _caller(pn2, "pn2_tile_labels", dict(n=100, num_class=9, votes=fake, labels=fake, stream=None))
    assert labels(n=0) == EINVAL and labels(num_class=0) == EINVAL and labels(num_class=65) == EUNSUP
    assert labels(votes=None) == ENULL and labels(labels=None) == ENULL
    assert labels(votes=odd(2)) == EINVAL and labels(labels=odd(1)) == EINVAL


def test_tile_cover_checks_its_arguments_before_the_device(pn2):
    rs = np.random.RandomState(0)
    p = np.stack([rs.uniform(0, 25, 50), rs.uniform(0, 15, 50), rs.uniform(0, 3, 50)], 1)
    ds = pn2.dataset.SemanticDataset(16, "test", False, 10, 10, "", device="cpu", scenes=[(p, None, None, "s")])
    with pytest.raises(ValueError, match="scene 1"):
        ds.tile_cover(1)
    with pytest.raises(ValueError, match="phase"):
        ds.tile_cover(0, phase=(-1.0, 0.0))
    with pytest.raises(ValueError, match="min_points"):
        ds.tile_cover(0, min_points=0)
    assert callable(pn2.predict.predict_scene_tiled)
