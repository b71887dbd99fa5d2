"""GPU tests of the tiled cover of a scene: pn2_tile_plan / pn2_tile_gather / pn2_tile_vote / pn2_tile_labels
(csrc/pn2_tile.hip) against the numpy model of the rule (tests/tile_ref.py), entry by entry and bit for bit, with every output and
the workspace between poisoned guards; SemanticDataset.tile_cover, predict.predict_scene_tiled and the --tiled route of
examples/predict_semantic3d.py.  Every comparison is exact."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tile_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64  # guard bytes in front of and behind every output (a multiple of 16: the table stays 16-byte aligned)
PHASES = [(0.0, 0.0), (5.0, 5.0), (2.5, 7.5)]


def _poisoned(torch, dev, nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=dev)


def _guarded(torch, dev, nbytes):
    """-> raw buffer, the view of its nbytes payload bytes"""
    raw = _poisoned(torch, dev, G + nbytes + G)
    return raw, raw[G:G + nbytes]


def _guards_intact(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _up(torch, dev, a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def _plan(pn2, dev, points, bx, by, npts, phase=(0.0, 0.0), min_points=1, cap=None):
    """one pn2_tile_plan call in poisoned surroundings -> dict like the model's (arrays read back; `samples` has all `cap`
    rows as raw bytes in "table"), after checking that nothing outside the outputs and the workspace was written and that the
    input did not change"""
    import torch
    launch, ptr = pn2._lib.launch, pn2._lib.ptr
    n = len(points)
    cap = n if cap is None else cap
    d_p = _up(torch, dev, points, np.float64)
    o_raw, o = _guarded(torch, dev, 4 * n)
    s_raw, s = _guarded(torch, dev, 16 * cap)
    h_raw, h = _guarded(torch, dev, 32)
    nbytes = ctypes.c_uint64(0)
    launch("pn2_tile_plan_workspace_size", dev, n, ctypes.byref(nbytes), stream=False)
    ws_raw = _poisoned(torch, dev, int(nbytes.value) + 512)
    off = (-ws_raw.data_ptr()) % 256
    ws = ws_raw[off:off + int(nbytes.value)]
    launch("pn2_tile_plan", dev, n, ptr(d_p), float(bx), float(by), phase[0], phase[1], npts, min_points, cap, ptr(o), ptr(s),
           ptr(h), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    wr = ws_raw.cpu().numpy()
    assert (wr[:off] == POISON).all() and (wr[off + int(nbytes.value):] == POISON).all(), "workspace guards"
    assert d_p.cpu().numpy().tobytes() == np.ascontiguousarray(points, dtype=np.float64).tobytes(), "the input changed"
    return dict(order=_guards_intact(o_raw, 4 * n, "order").view(np.int32), header=_guards_intact(h_raw, 32, "header").view(np.int32),
                table=_guards_intact(s_raw, 16 * cap, "samples"))


def _same_plan(got, want, cap):
    """the header, order and every table row equal the model's; table rows beyond the last sample keep their poison"""
    assert got["header"].tolist() == want["header"].tolist()
    assert np.array_equal(got["order"], want["order"])
    rows = len(want["samples"])
    assert rows == min(int(want["header"][1]), cap)
    assert np.array_equal(got["table"][:16 * rows].view(np.int32).reshape(-1, 4), want["samples"])
    assert (got["table"][16 * rows:] == POISON).all(), "a table row beyond the last sample"


# ---- geometries: (points sorted by x, box_size_x, box_size_y) -------------------------------------------------------------------
def _uniform(n, seed=0):
    """uniform in 25 m x 15 m, boxes of 10 m; z >= 0 with zeros of both signs among the smallest"""
    rs = np.random.RandomState(1000 + n + seed)
    z = np.abs(rs.normal(0, 1.5, n))
    z[rs.permutation(n)[:max(1, n // 7)]] = np.where(rs.randint(0, 2, max(1, n // 7)) == 1, -0.0, 0.0)
    return np.stack([np.sort(rs.uniform(0, 25, n)), rs.uniform(0, 15, n), z], 1), 10.0, 10.0


def _lattice(n, seed=0):
    """coordinates that are multiples of 2 in [-16, 16], box 8: every quotient is exact, negatives and exact boundaries included"""
    rs = np.random.RandomState(2000 + n + seed)
    return np.stack([np.sort(rs.randint(-8, 9, n) * 2.0), rs.randint(-8, 9, n) * 2.0, rs.randint(0, 4, n) * 0.5], 1), 8.0, 8.0


def _identical(n, seed=0):
    return np.tile(np.array([[1.5, -2.25, 0.5]]), (n, 1)), 10.0, 10.0


def _own_tile(n, seed=0):
    """every point its own tile: x steps by two boxes of 2^-10 m"""
    rs = np.random.RandomState(3000 + n + seed)
    return np.stack([np.arange(n) * 2.0 ** -9, rs.randint(0, 1 << 14, n) * 2.0 ** -10, rs.uniform(0, 3, n)], 1), 2.0 ** -10, 2.0 ** -10


def _equal_x_runs(n, seed=0):
    """eight values of x: long runs of equal x whose members differ in y, so the tile order reshuffles them"""
    rs = np.random.RandomState(4000 + n + seed)
    return np.stack([np.sort(rs.randint(0, 8, n) * 3.5), rs.uniform(0, 15, n), rs.uniform(0, 3, n)], 1), 10.0, 10.0


GEOMETRIES = dict(uniform=_uniform, lattice=_lattice, identical=_identical, own_tile=_own_tile, equal_x_runs=_equal_x_runs)
# one below, at and one above: a wave (64), a workgroup / one ordered pass (kT = 256), a chunk of positions or of tiles
# (kChunk = 1024; own_tile makes the tiles as many as the points), 4097 for several chunks
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
# the one-workgroup scan over the chunks takes more than one chunk per thread above kScanT = 256 chunks of 1024
SCAN_SIZES = [256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_plan_equals_the_model_entry_by_entry(pn2, cuda, geometry, n):
    """order, every table row and the header, for N = 4 and 64 and three phases.  The sizes stand one below, at and one above
    the block sizes of csrc/pn2_tile.hip: a wave (64: the ballots and shuffles of its scans), a workgroup and one ordered pass
    of a compaction (kT = 256), a chunk (kChunk = 1024 sorted positions in the head count and emit, 1024 tiles in the sample
    count and the row emit -- own_tile has as many tiles as points), and several chunks (4097).  The scan over the chunks
    (kScanT = 256 threads, one chunk each up to 256 chunks) has its own test below."""
    p, bx, by = GEOMETRIES[geometry](n)
    for npts in (4, 64):
        for ph in PHASES:
            want = M.plan(p, bx, by, npts, ph)
            assert want["header"][3] == 0 and want["header"][2] == 0
            _same_plan(_plan(pn2, cuda, p, bx, by, npts, ph), want, n)


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("geometry", ["uniform", "own_tile"])
def test_plan_beyond_one_chunk_per_scan_thread(pn2, cuda, geometry, n):
    """256 chunks and 257: positions (both geometries) and tiles (own_tile) on both sides of the scan's one-chunk-per-thread"""
    p, bx, by = GEOMETRIES[geometry](n)
    want = M.plan(p, bx, by, 4, PHASES[1])
    assert want["header"][3] == 0 and want["header"][0] == (n if geometry == "own_tile" else want["header"][0])
    _same_plan(_plan(pn2, cuda, p, bx, by, 4, PHASES[1]), want, n)


def test_plan_statuses_and_min_points(pn2, cuda):
    p, bx, by = _uniform(1025)
    q = p.copy()
    q[700, 1] = np.nan
    assert M.plan(q, bx, by, 64)["header"][3] == 1
    assert _plan(pn2, cuda, q, bx, by, 64)["header"][3] == 1  # (and nothing outside the outputs was written)
    # a table that is too small: status 3, n_samples still the true total, the first sample_cap rows written
    want = M.plan(p, bx, by, 4, sample_cap=100)
    assert want["header"][3] == 3 and want["header"][1] > 100 and len(want["samples"]) == 100
    _same_plan(_plan(pn2, cuda, p, bx, by, 4, cap=100), want, 100)
    got = _plan(pn2, cuda, p, bx, by, 4, cap=0)  # counting only
    assert got["header"].tolist() == want["header"].tolist()
    # a tile index of 2^31
    r = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert M.plan(r, 2.0 ** -31, 10, 4)["header"][3] == 2 and _plan(pn2, cuda, r, 2.0 ** -31, 10, 4)["header"][3] == 2
    # min_points above the smallest tile(s): they are skipped and counted
    sizes = M.plan(p, bx, by, 1 << 20)["samples"][:, 1]
    k = int(np.sort(sizes)[1]) + 1  # skips at least the two smallest tiles
    want = M.plan(p, bx, by, 64, PHASES[2], min_points=k)
    assert want["header"][2] > 0 and want["header"][1] > 0
    _same_plan(_plan(pn2, cuda, p, bx, by, 64, PHASES[2], min_points=k), want, 1025)
    want = M.plan(p, bx, by, 64, min_points=2000)  # every tile
    assert want["header"].tolist()[:4] == [want["header"][0], 0, 1025, 0]
    _same_plan(_plan(pn2, cuda, p, bx, by, 64, min_points=2000), want, 1025)


# ---- gather -----------------------------------------------------------------------------------------------------------------
def _gather(pn2, dev, pl, points, colors, q0, b, npts, bx, by):
    """one pn2_tile_gather call on the MODEL's plan, outputs between guards -> data, sel, live as arrays"""
    import torch
    launch, ptr = pn2._lib.launch, pn2._lib.ptr
    ch = 3 if colors is None else 6
    d_p, d_c = _up(torch, dev, points, np.float64), _up(torch, dev, colors, np.float32)
    d_o, d_h = _up(torch, dev, pl["order"], np.int32), _up(torch, dev, pl["header"], np.int32)
    table = pl["samples"] if len(pl["samples"]) else np.full((1, 4), 0x5A5A5A5A, dtype=np.int32)  # never read
    d_s = _up(torch, dev, table, np.int32)
    sizes = dict(data=4 * b * npts * ch, sel=4 * b * npts, live=4 * b)
    bufs = {k: _guarded(torch, dev, v) for k, v in sizes.items()}
    launch("pn2_tile_gather", dev, b, npts, q0, int(colors is not None), ptr(d_p), ptr(d_c), ptr(d_o), ptr(d_s), ptr(d_h), float(bx),
           float(by), ptr(bufs["data"][1]), ptr(bufs["sel"][1]), ptr(bufs["live"][1]))
    torch.cuda.synchronize()
    out = {k: _guards_intact(bufs[k][0], sizes[k], k) for k in sizes}
    return out["data"].view(np.float32).reshape(b, npts, ch), out["sel"].view(np.int32).reshape(b, npts), out["live"].view(np.int32)


def _same_batch(got, want):
    for g, w, name in zip(got, want, ("data", "sel", "live")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("npts, n", [(4, 257), (64, 4097), (1025, 4097)])  # (1025: a sample shared by two workgroups)
@pytest.mark.parametrize("colour", [False, True])
def test_gather_equals_the_model_bit_for_bit(pn2, cuda, npts, n, colour):
    p, bx, by = _uniform(n, seed=1)
    col = np.random.RandomState(n).random_sample((n, 3)).astype(np.float32) if colour else None
    pl = M.plan(p, bx, by, npts, PHASES[1])
    ns = int(pl["header"][1])
    assert ns >= 4
    for b in (1, 3):
        for q0 in (0, ns // 2, ns - 2, ns - 1, ns, ns + 5):  # inside the table, across its end, wholly beyond it
            want = M.batch(pl, p, col, q0, b, npts, bx, by)
            assert (want[2] > 0).sum() == max(0, min(b, ns - q0))
            _same_batch(_gather(pn2, cuda, pl, p, col, q0, b, npts, bx, by), want)
    # negative coordinates, exact boundaries, minima that are zeros
    p, bx, by = _lattice(n)
    p[:, 2] -= 0.5
    pl = M.plan(p, bx, by, npts, PHASES[0])
    _same_batch(_gather(pn2, cuda, pl, p, col, 0, 3, npts, bx, by), M.batch(pl, p, col, 0, 3, npts, bx, by))


def test_gather_without_samples_is_zero_filled(pn2, cuda):
    p, bx, by = _uniform(257)
    col = np.random.RandomState(1).random_sample((257, 3)).astype(np.float32)
    pl = M.plan(p, bx, by, 64, min_points=1000)
    assert pl["header"][1] == 0
    for c in (None, col):
        got = _gather(pn2, cuda, pl, p, c, 0, 3, 64, bx, by)
        _same_batch(got, M.batch(pl, p, c, 0, 3, 64, bx, by))
        assert not got[0].any() and (got[1] == -1).all() and not got[2].any()
    # a plan that was refused offers no sample either
    pl = M.plan(p, bx, by, 64)
    pl["header"][3] = 3
    got = _gather(pn2, cuda, pl, p, None, 0, 1, 64, bx, by)
    assert not got[0].any() and (got[1] == -1).all() and not got[2].any()


# ---- vote, labels -----------------------------------------------------------------------------------------------------------
def _vote(pn2, dev, votes, sel, live, pred, dropped=None):
    launch, ptr = pn2._lib.launch, pn2._lib.ptr
    b, npts = sel.shape
    launch("pn2_tile_vote", dev, b, npts, votes.shape[1], ptr(sel), ptr(live), ptr(pred), ptr(votes), ptr(dropped))


def _labels(pn2, dev, votes):
    import torch
    raw, lab = _guarded(torch, dev, 4 * votes.shape[0])
    pn2._lib.launch("pn2_tile_labels", dev, votes.shape[0], votes.shape[1], pn2._lib.ptr(votes), pn2._lib.ptr(lab))
    torch.cuda.synchronize()
    return _guards_intact(raw, 4 * votes.shape[0], "labels").view(np.int32)


def test_vote_and_labels_equal_the_model(pn2, cuda):
    import torch
    n, npts, b, C = 1025, 64, 3, 9
    p, bx, by = _uniform(n, seed=2)
    rs = np.random.RandomState(5)
    want_votes = np.zeros((n, C), dtype=np.int32)
    raw, payload = _guarded(torch, cuda, 4 * n * C)
    payload.zero_()
    votes = payload.view(torch.int32).reshape(n, C)
    dropped = torch.zeros(1, dtype=torch.int64, device=cuda)
    want_dropped = 0
    for ph in PHASES[:2]:
        pl = M.plan(p, bx, by, npts, ph)
        for q0 in range(0, int(pl["header"][1]), b):
            _, sel, live = M.batch(pl, p, None, q0, b, npts, bx, by)
            pred = rs.randint(-1, C + 1, (b, npts)).astype(np.int32)  # -1 and C are out of range
            want_dropped += M.vote(want_votes, sel, live, pred)
            _vote(pn2, cuda, votes, _up(torch, cuda, sel, np.int32), _up(torch, cuda, live, np.int32), _up(torch, cuda, pred, np.int32),
                  dropped)
    torch.cuda.synchronize()
    assert want_dropped > 0 and int(dropped.item()) == want_dropped
    got = _guards_intact(raw, 4 * n * C, "votes").view(np.int32).reshape(n, C)
    assert np.array_equal(got, want_votes)
    assert (want_votes.sum(1) == 0).any() and (want_votes.sum(1) == 2).any()  # points without a vote, points with both
    lab = _labels(pn2, cuda, votes)
    assert np.array_equal(lab, M.labels(want_votes))
    assert (lab[want_votes.sum(1) == 0] == 0).all()
    # without a counter the same votes; ties resolve to the lowest class
    v2 = torch.zeros((4, C), dtype=torch.int32, device=cuda)
    sel = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 0]], dtype=torch.int32, device=cuda)
    pred = torch.tensor([[5, 8, 0, C], [2, 8, 7, 5]], dtype=torch.int32, device=cuda)
    _vote(pn2, cuda, v2, sel, torch.tensor([4, 3], dtype=torch.int32, device=cuda), pred)
    assert v2.cpu().numpy().tolist() == [[0, 0, 1, 0, 0, 1, 0, 0, 0], [0] * 8 + [2], [1, 0, 0, 0, 0, 0, 0, 1, 0], [0] * 9]
    assert _labels(pn2, cuda, v2).tolist() == [2, 8, 0, 0]


def test_every_point_gets_one_vote_per_pass(pn2, cuda):
    """the model-independent invariant, on the device's own plan and batches: after P passes with min_points = 1 every point
    holds exactly P votes.  The feed is every batch of every pass."""
    import torch
    launch, ptr = pn2._lib.launch, pn2._lib.ptr
    n, npts, b, C = 4097, 64, 3, 9
    p, bx, by = _uniform(n, seed=3)
    ds = pn2.dataset.SemanticDataset(npts, "test", False, bx, by, "", device=cuda, scenes=[(p, None, None, "s")])
    votes = torch.zeros((n, C), dtype=torch.int32, device=cuda)
    dropped = torch.zeros(1, dtype=torch.int64, device=cuda)
    gen = torch.Generator(device="cpu").manual_seed(1)
    for P, ph in enumerate(PHASES, 1):
        cover = ds.tile_cover(0, ph)
        want = M.plan(p, bx, by, npts, ph)
        assert (cover.num_tiles, cover.num_samples, cover.skipped_points) == tuple(want["header"][:3].tolist())
        assert cover.skipped_points == 0 and tuple(cover.samples.shape) == (cover.num_samples, 4)
        for q0 in range(0, cover.num_samples, b):
            data, sel, live = cover.batch(q0, b)
            assert tuple(data.shape) == (b, npts, 3) and tuple(sel.shape) == (b, npts) and tuple(live.shape) == (b,)
            pred = torch.randint(0, C, (b, npts), generator=gen, dtype=torch.int32).to(cuda)
            launch("pn2_tile_vote", cuda, b, npts, C, ptr(sel), ptr(live), ptr(pred), ptr(votes), ptr(dropped))
        assert (votes.sum(1) == P).all()
    assert int(dropped.item()) == 0


# ---- the dataset, end to end ------------------------------------------------------------------------------------------------
B, N, C = 8, 2048, 9
E2E_PHASES = ((0.0, 0.0), (5.0, 5.0))


def _scene(n=20000, seed=7):
    """20 000 points over 25 m x 15 m, float32 values as a .pcd holds them; x distinct (the host store's sort leaves the order of
    equal x open)"""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.permutation(n) * 0.00125, rs.uniform(0, 15, n), np.abs(rs.normal(0, 1.5, n))], 1).astype(np.float32).astype(np.float64)
    return pts, rs.randint(0, C, n).astype(np.int32), rs.randint(0, 256, (n, 3)) / 255.0


@pytest.fixture(scope="module")
def predictor(pn2, cuda):
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(num_point=N, l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)
    return pn2.predict.Predictor(None, C, hp, device=cuda, seed=5)


def test_predict_scene_tiled_equals_the_hand_written_loop(pn2, cuda, predictor):
    import torch
    pts, lab, col = _scene()
    ds = pn2.dataset.SemanticDataset(N, "validation", True, 10, 10, "", device=cuda, scenes=[(pts, lab, col, "s")])
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    assert not predictor._graphs
    labels, votes = pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=B, phases=E2E_PHASES, confusion=cm)
    assert len(predictor._graphs) == 1 and (B, N) in predictor._graphs  # the padded last batches kept the one shape
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (20000,) and labels.is_cuda
    assert votes.dtype == torch.int32 and tuple(votes.shape) == (20000, C)
    sp, sc, sl = ds.scene_points[0], ds.scene_colors[0].astype(np.float32), ds.scene_labels[0]
    second = M.plan(sp, 10, 10, N, E2E_PHASES[1])
    assert second["header"][1] > B and second["header"][1] % B != 0  # two batches at least, the last one padded
    predict = lambda data: predictor.predict(torch.from_numpy(data).to(cuda)).cpu().numpy()  # noqa: E731
    want_labels, want_votes = M.predict_scene(sp, sc, 10, 10, N, C, predict, B, phases=E2E_PHASES)
    assert np.array_equal(votes.cpu().numpy(), want_votes) and np.array_equal(labels.cpu().numpy(), want_labels)
    assert (want_votes.sum(1) == 2).all() and len(np.unique(want_labels)) > 1
    assert len(predictor._graphs) == 1
    g, p = sl.astype(np.int64), want_labels.astype(np.int64)
    assert np.array_equal(cm.confusion_matrix.reshape(-1), np.bincount(g * C + p, minlength=C * C))
    assert cm.confusion_matrix.sum() == 20000
    # the store built on the device gives the same cover and the same labels, and scene_perm carries them to input order
    dd = pn2.dataset.SemanticDataset(N, "validation", True, 10, 10, "", device=cuda, scenes=[(pts, lab, col, "s")], ingest="device",
                                     keep_perm=True)
    a, b = ds.tile_cover(0, E2E_PHASES[1], min_points=3), dd.tile_cover(0, E2E_PHASES[1], min_points=3)
    assert (a.num_tiles, a.num_samples, a.skipped_points) == (b.num_tiles, b.num_samples, b.skipped_points)
    assert torch.equal(a.order, b.order) and torch.equal(a.samples, b.samples)
    for x, y in zip(a.batch(B, B), b.batch(B, B)):
        assert torch.equal(x, y)
    labels2, votes2 = pn2.predict.predict_scene_tiled(predictor, dd, 0, batch_size=B, phases=E2E_PHASES)
    assert torch.equal(labels2, labels) and torch.equal(votes2, votes)
    back = torch.empty_like(labels2)
    back[dd.scene_perm[0].long()] = labels2
    assert np.array_equal(back.cpu().numpy()[np.argsort(pts[:, 0], kind="stable")], want_labels)
    with pytest.raises(ValueError):
        pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=0)
    q = pts.copy()
    q[5, 1] = np.inf
    bad = pn2.dataset.SemanticDataset(N, "test", False, 10, 10, "", device=cuda, scenes=[(q, None, None, "broken")])
    with pytest.raises(ValueError, match="'broken'.*non-finite"):
        bad.tile_cover(0)


@pytest.mark.timeout(300)
def test_example_tiled_route_agrees_with_the_in_memory_call(pn2, cuda, tmp_path):
    import torch
    U = pn2.util.point_cloud_util
    path = os.path.join(ROOT, "examples", "predict_semantic3d.py")
    flags = ["--tiled", "--phases", "2", "--min-points", "2", "--batch-size", str(B), "--points", str(N), "--npoint", "256,64,32,16",
             "--scenes", "1", "--scene-points", "30000", "--voxel", "0.1", "--chunk", "25000"]
    run = subprocess.run([sys.executable, path] + flags, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    assert "2 grid(s) of columns" in out and "Sparse results" in out and "Global results" in out
    # the same scene, store and predictor in this process
    spec = importlib.util.spec_from_file_location("predict_semantic3d_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.setdefault("box_size_x", 10)
    hp.setdefault("box_size_y", 10)
    hp.update(use_color=1, num_point=N, l1_npoint=256, l2_npoint=64, l3_npoint=32, l4_npoint=16)

    class Args:
        data, raw, set, scenes, scene_points, voxel, ingest = None, None, "validation", 1, 30000, 0.1, "host"
    ds, dense = ex.load_scenes(Args, hp, cuda)
    pred = pn2.predict.Predictor(None, ds.num_classes, hp, device=cuda)
    phases = ((0.0, 0.0), (hp["box_size_x"] / 2, hp["box_size_y"] / 2))
    labels, votes = pn2.predict.predict_scene_tiled(pred, ds, 0, batch_size=B, phases=phases, min_points=2)
    name = "syn_validation_0"
    sp, _ = U.read_point_cloud_pcd(str(tmp_path / "result" / "sparse" / (name + ".pcd")))
    sl = U.load_labels(str(tmp_path / "result" / "sparse" / (name + ".labels")))
    assert sp.shape == (len(ds.scene_points[0]), 3) and np.array_equal(sp.astype(np.float32), ds.scene_points[0].astype(np.float32))
    assert np.array_equal(sl, labels.cpu().numpy())
    dl = U.load_labels(str(tmp_path / "result" / "dense" / (name + ".labels")))
    lab, _ = pn2.predict.label_dense(torch.from_numpy(sp.astype(np.float32)).to(cuda), labels, dense[name][0])
    assert dl.shape == (30000,) and np.array_equal(lab.cpu().numpy(), dl)
