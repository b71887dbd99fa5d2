"""GPU tests of soft voting: pn2_softmax_scores / pn2_tile_vote_scores / pn2_score_labels (csrc/pn2_soft_vote.hip) and
pn2_interpolate_scores (csrc/pn2_label_interp.hip) against the numpy model of the rules (tests/soft_vote_ref.py), with every
output between poisoned guards and the inputs unchanged; Predictor.predict_scores, predict_scene_tiled(vote="soft"),
label_dense_scores and the --soft route of examples/predict_semantic3d.py.

The only tolerance is the softmax's one unit of 2^-30: the device's exp and numpy's are each within about an ulp of float64, so
p * 2^30 differs between them by far less than 2^-20 units, and the rounded integers can differ only where that value lies that
close to a half-integer -- then by one.  Everything downstream takes q as its input and is compared exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import soft_vote_ref as S  # noqa: E402
import tile_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5
G = 64  # guard bytes in front of and behind every output


def _guarded(torch, dev, nbytes, zero=False):
    """-> raw buffer, the view of its nbytes payload bytes"""
    raw = torch.full((G + nbytes + G,), POISON, dtype=torch.uint8, device=dev)
    if zero:
        raw[G:G + nbytes].zero_()
    return raw, raw[G:G + nbytes]


def _payload(raw, nbytes, what):
    h = raw.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[G + nbytes:] == POISON).all(), "%s: written outside its bounds" % what
    return h[G:G + nbytes]


def _up(torch, dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def _unchanged(t, a, dt, what):
    assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a, dtype=dt).tobytes(), "%s changed" % what


# ---- softmax ----------------------------------------------------------------------------------------------------------------
def _softmax(pn2, dev, x, invalid=None):
    """one pn2_softmax_scores call -> q (rows,C) int32, the invalid count (of `invalid`, a counter that is carried on)"""
    import torch
    rows, C = x.shape
    d_x = _up(torch, dev, x, np.float32)
    raw, q = _guarded(torch, dev, 4 * rows * C)
    invalid = torch.zeros(1, dtype=torch.int64, device=dev) if invalid is None else invalid
    pn2._lib.launch("pn2_softmax_scores", dev, rows, C, pn2._lib.ptr(d_x), pn2._lib.ptr(q), pn2._lib.ptr(invalid))
    torch.cuda.synchronize()
    _unchanged(d_x, x, np.float32, "logits")
    return _payload(raw, 4 * rows * C, "q").view(np.int32).reshape(rows, C), int(invalid.item())


@pytest.mark.parametrize("C", [1, 2, 9, 13, 64])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 1000])
def test_softmax_scores_within_one_unit_of_the_model(pn2, cuda, rows, C):
    rs = np.random.RandomState(rows * 100 + C)
    x = (rs.standard_normal((rows, C)) * rs.choice([0.1, 3.0, 30.0], (rows, 1))).astype(np.float32)
    want, _ = S.softmax_scores(x)
    q, invalid = _softmax(pn2, cuda, x)
    assert invalid == 0 and (q >= 0).all()
    assert np.abs(q.astype(np.int64) - want).max() <= 1
    assert np.abs(q.astype(np.int64).sum(1) - S.ONE).max() <= C / 2 + 1
    # monotone, exactly: the largest logit holds the largest score
    assert (q[np.arange(rows), np.argmax(x, 1)] == q.max(1)).all()


def test_softmax_scores_exact_cases(pn2, cuda):
    inf, nan = np.inf, np.nan
    for C in (2, 4, 8):  # equal logits: e = 1, s = C, p = 1 / C, all exact
        x = np.repeat(np.array([[0.0], [-7.25], [1e30], [-3e38]], dtype=np.float32), C, axis=1)
        q, invalid = _softmax(pn2, cuda, x)
        assert invalid == 0 and (q == S.ONE // C).all()
    # one logit more than 800 above the rest: exp(-800) is 0 in float64
    x = np.array([[900.5, 100, -3, 0, 99.5], [0, -801, -1e4, -3e38, -900]], dtype=np.float32)
    q, invalid = _softmax(pn2, cuda, x)
    assert invalid == 0 and q.tolist() == [[S.ONE, 0, 0, 0, 0]] * 2
    # -inf entries of a finite row are p = 0 (the finite ones equal: exact); NaN, +inf and all -inf rows are zero and counted
    x = np.array([[5, -inf, 5, -inf], [-inf, -inf, 2, -inf], [-inf, 1, 1, 1 - 801],
                  [nan, 0, 0, 0], [0, 0, 0, nan], [0, inf, 0, 0], [inf, inf, inf, inf], [-inf] * 4, [nan, inf, -inf, 0]], dtype=np.float32)
    q, invalid = _softmax(pn2, cuda, x)
    assert invalid == 6
    assert q.tolist() == [[1 << 29, 0, 1 << 29, 0], [0, 0, S.ONE, 0], [0, 1 << 29, 1 << 29, 0]] + [[0] * 4] * 6
    want, wi = S.softmax_scores(x)
    assert wi == 6 and np.array_equal(want, q)
    import torch
    counter = torch.full((1,), 1 << 40, dtype=torch.int64, device=cuda)  # the counter accumulates and is never zeroed
    assert _softmax(pn2, cuda, x, counter)[1] == (1 << 40) + 6 and _softmax(pn2, cuda, x[2:6], counter)[1] == (1 << 40) + 9
    # -inf among unequal finite logits: zero there, the rest within a unit
    rs = np.random.RandomState(3)
    x = (rs.standard_normal((257, 9)) * 4).astype(np.float32)
    x[rs.random_sample(x.shape) < 0.3] = -inf
    x[:, 0] = rs.standard_normal(257)  # no row is all -inf
    q, invalid = _softmax(pn2, cuda, x)
    want, _ = S.softmax_scores(x)
    assert invalid == 0 and (q[np.isinf(x)] == 0).all() and np.abs(q.astype(np.int64) - want).max() <= 1


# ---- vote, labels -----------------------------------------------------------------------------------------------------------
def _vote(pn2, dev, scores, sel, live, q, dropped):
    import torch
    ptr = pn2._lib.ptr
    b, npts, C = q.shape
    d = [_up(torch, dev, a, np.int32) for a in (sel, live, q)]
    pn2._lib.launch("pn2_tile_vote_scores", dev, b, npts, C, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(scores), ptr(dropped))
    torch.cuda.synchronize()
    for t, a, name in zip(d, (sel, live, q), ("sel", "live", "q")):
        _unchanged(t, a, np.int32, name)


def _score_labels(pn2, dev, scores, confidence=True):
    """scores: a device (n,C) int64 tensor -> labels, confidence (or None) as arrays"""
    import torch
    n, C = scores.shape
    before = scores.cpu().numpy().copy()
    lraw, lab = _guarded(torch, dev, 4 * n)
    craw, conf = _guarded(torch, dev, 4 * n)
    pn2._lib.launch("pn2_score_labels", dev, n, C, pn2._lib.ptr(scores), pn2._lib.ptr(lab), pn2._lib.ptr(conf) if confidence else None)
    torch.cuda.synchronize()
    assert np.array_equal(scores.cpu().numpy(), before)
    c = _payload(craw, 4 * n, "confidence")
    if not confidence:
        assert (c == POISON).all()
    return _payload(lraw, 4 * n, "labels").view(np.int32), (c.view(np.float32) if confidence else None)


@pytest.mark.parametrize("b, npts, n, C", [(1, 1, 50, 1), (2, 64, 100, 9), (3, 100, 300, 13), (4, 257, 500, 64)])
def test_vote_scores_and_labels_equal_the_model(pn2, cuda, b, npts, n, C):
    """three launches into one table: every sample is not live at all, partly live and fully live once; some rows aim at no
    point (sel = -1) and some hold a negative entry: dropped whole and counted"""
    import torch
    rs = np.random.RandomState(b * 1000 + npts)
    raw, payload = _guarded(torch, cuda, 8 * n * C, zero=True)
    scores = payload.view(torch.int64).reshape(n, C)
    dropped = torch.zeros(1, dtype=torch.int64, device=cuda)
    want = np.zeros((n, C), dtype=np.int64)
    want_dropped = 0
    kinds = [0, (npts + 1) // 2, npts]
    for launch in range(3):
        live = np.array([kinds[(s + launch) % 3] for s in range(b)], dtype=np.int32)
        sel = rs.randint(0, n, (b, npts)).astype(np.int32)
        sel[rs.random_sample(sel.shape) < 0.1] = -1
        q = rs.randint(0, S.ONE + 1, (b, npts, C)).astype(np.int32)
        q[rs.random_sample(q.shape) < 0.2] = 0
        neg = rs.random_sample((b, npts)) < 0.1
        q[neg, rs.randint(0, C, int(neg.sum()))] = -rs.randint(1, 1 << 30, int(neg.sum()))
        want_dropped += S.vote_scores(want, sel, live, q)
        _vote(pn2, cuda, scores, sel, live, q, dropped)
    assert int(dropped.item()) == want_dropped and (want_dropped > 0 or npts == 1)
    got = _payload(raw, 8 * n * C, "scores").view(np.int64).reshape(n, C)
    assert np.array_equal(got, want) and (want.sum() > 0 or npts == 1)
    assert (want.sum(1) == 0).any()  # points nobody voted for
    lab, conf = _score_labels(pn2, cuda, scores)
    wl, wc = S.score_labels(want)
    assert np.array_equal(lab, wl) and conf.tobytes() == wc.tobytes()
    assert (lab[want.sum(1) == 0] == 0).all() and (conf[want.sum(1) == 0] == 0).all()


def test_vote_scores_many_rows_on_one_point(pn2, cuda):
    """4096 live rows all aimed at point 7: the 64-bit atomics give the exact sum, beyond what an int32 holds"""
    import torch
    rs = np.random.RandomState(9)
    b, npts, n, C = 4, 1024, 16, 9
    q = rs.randint(0, S.ONE + 1, (b, npts, C)).astype(np.int32)
    sel = np.full((b, npts), 7, dtype=np.int32)
    live = np.full(b, npts, dtype=np.int32)
    raw, payload = _guarded(torch, cuda, 8 * n * C, zero=True)
    _vote(pn2, cuda, payload.view(torch.int64).reshape(n, C), sel, live, q, None)  # no counter
    got = _payload(raw, 8 * n * C, "scores").view(np.int64).reshape(n, C)
    want = np.zeros((n, C), dtype=np.int64)
    want[7] = q.astype(np.int64).sum(axis=(0, 1))
    assert np.array_equal(got, want) and (want[7] > 1 << 40).all()


def test_score_labels_ties_zero_rows_and_large_sums(pn2, cuda):
    import torch
    big = 1 << 57
    rows = [[0, 0, 0, 0], [5, 5, 0, 0], [0, 7, 7, 7], [1, 2, 3, 3], [big, 1, big, 0], [0, 0, 0, 1], [3, 0, 0, 0], [1, 1, 1, 1],
            [big - 1, big, big, big - 1]]
    rs = np.random.RandomState(2)
    sc = np.concatenate([np.array(rows, dtype=np.int64), rs.randint(0, 3, (300, 4)).astype(np.int64),
                         rs.randint(0, 1 << 62, (300, 4), dtype=np.int64) >> rs.randint(4, 60, (300, 1))])
    wl, wc = S.score_labels(sc)
    assert wl[:9].tolist() == [0, 0, 1, 2, 0, 3, 0, 0, 1] and wc[0] == 0 and wc[7] == 0.25
    lab, conf = _score_labels(pn2, cuda, _up(torch, cuda, sc, np.int64))
    assert np.array_equal(lab, wl) and conf.tobytes() == wc.tobytes()
    lab, conf = _score_labels(pn2, cuda, _up(torch, cuda, sc, np.int64), confidence=False)
    assert np.array_equal(lab, wl) and conf is None
    for C in (1, 64):  # the narrowest and the widest row
        sc = rs.randint(0, 4, (257, C)).astype(np.int64) << 31
        lab, conf = _score_labels(pn2, cuda, _up(torch, cuda, sc, np.int64))
        wl, wc = S.score_labels(sc)
        assert np.array_equal(lab, wl) and conf.tobytes() == wc.tobytes()


# ---- the dense step ---------------------------------------------------------------------------------------------------------
def _geometry(kind, ns, nd, seed):
    """-> sparse (ns,3), dense (nd,3) float32"""
    rs = np.random.RandomState(seed)
    dp = rs.uniform(0, 10, (nd, 3))
    if kind == "uniform":
        sp = rs.uniform(0, 10, (ns, 3))
    elif kind == "duplicated":  # every point several times: the index decides
        sp = rs.uniform(0, 10, (max(1, ns // 4), 3))[rs.randint(0, max(1, ns // 4), ns)]
    elif kind == "identical":
        sp = np.tile(np.array([[1.5, -2.25, 0.5]]), (ns, 1))
    elif kind == "collinear":
        sp = np.outer(rs.randint(0, 50, ns) * 0.25, [1.0, 2.0, -0.5])
        dp[::2] = np.outer(rs.uniform(0, 12, len(dp[::2])), [1.0, 2.0, -0.5])
    else:  # "far": the dense points far outside the sparse bounding box, on every side
        sp = rs.uniform(0, 1, (ns, 3))
        dp = rs.uniform(-1, 1, (nd, 3)) * 1000.0 + rs.choice([-5000.0, 0.0, 5000.0], (nd, 3))
    return sp.astype(np.float32), dp.astype(np.float32)


def _dense(pn2, dev, sp, sc, dp, knn, confidence=True):
    """one pn2_interpolate_scores call in poisoned surroundings -> labels, colours, confidence as arrays"""
    import torch
    ptr = pn2._lib.ptr
    ns, nd, C = len(sp), len(dp), sc.shape[1]
    d_sp, d_dp, d_sc = _up(torch, dev, sp, np.float32), _up(torch, dev, dp, np.float32), _up(torch, dev, sc, np.int64)
    lraw, lab = _guarded(torch, dev, 4 * nd)
    kraw, col = _guarded(torch, dev, 3 * nd)
    craw, conf = _guarded(torch, dev, 4 * nd)
    wbytes = int(pn2._lib.lib.pn2_interpolate_label_workspace_bytes(ns))
    ws_raw = torch.full((wbytes + 512,), POISON, dtype=torch.uint8, device=dev)
    off = (-ws_raw.data_ptr()) % 256
    pn2._lib.launch("pn2_interpolate_scores", dev, ns, nd, C, ptr(d_sp), ptr(d_sc), ptr(d_dp), ptr(lab), ptr(col),
                    ptr(conf) if confidence else None, knn, ptr(ws_raw, off), wbytes)
    torch.cuda.synchronize()
    assert (ws_raw[:off] == POISON).all() and (ws_raw[off + wbytes:] == POISON).all(), "workspace guards"
    _unchanged(d_sp, sp, np.float32, "sparse_points")
    _unchanged(d_dp, dp, np.float32, "dense_points")
    _unchanged(d_sc, sc, np.int64, "sparse_scores")
    c = _payload(craw, 4 * nd, "confidence")
    if not confidence:
        assert (c == POISON).all()
    return (_payload(lraw, 4 * nd, "labels").view(np.int32), _payload(kraw, 3 * nd, "colors").reshape(nd, 3),
            c.view(np.float32) if confidence else None)


DENSE_CASES = [  # ns, nd, knn, C, geometry
    (1, 1, 1, 1, "uniform"), (1, 255, 3, 9, "uniform"), (2, 257, 3, 9, "duplicated"), (2, 255, 16, 64, "uniform"),
    (3, 257, 4, 9, "collinear"), (3, 3000, 5, 1, "identical"), (17, 255, 16, 9, "uniform"), (17, 257, 5, 64, "duplicated"),
    (17, 1, 3, 9, "far"), (1000, 3000, 3, 9, "uniform"), (1000, 257, 16, 9, "far"), (1000, 255, 4, 64, "identical"),
    (1000, 257, 5, 9, "collinear"), (5000, 3000, 3, 9, "uniform"), (5000, 257, 5, 9, "duplicated"), (5000, 255, 1, 9, "collinear"),
    (5000, 1, 16, 64, "far"), (5000, 257, 4, 1, "uniform"),
]


@pytest.mark.parametrize("ns, nd, knn, C, kind", DENSE_CASES)
def test_interpolate_scores_equals_the_model(pn2, cuda, ns, nd, knn, C, kind):
    sp, dp = _geometry(kind, ns, nd, seed=ns + nd + knn)
    rs = np.random.RandomState(ns * 7 + C)
    sc = rs.randint(0, 1 << 32, (ns, C), dtype=np.int64)
    sc[rs.random_sample(ns) < 0.1] = 0  # sparse points nobody voted for
    wl, wk, wc = S.interpolate_scores(sp, sc, dp, knn)
    lab, col, conf = _dense(pn2, cuda, sp, sc, dp, knn)
    assert np.array_equal(lab, wl) and np.array_equal(col, wk) and conf.tobytes() == wc.tobytes()


def test_interpolate_scores_edges(pn2, cuda):
    import torch
    sp, dp = _geometry("uniform", 17, 257, seed=1)
    sc = np.zeros((17, 9), dtype=np.int64)
    lab, col, conf = _dense(pn2, cuda, sp, sc, dp, 3)  # all zero: label 0, its colour, confidence 0
    assert (lab == 0).all() and (col == 255).all() and (conf == 0).all()
    sc[:, 4] = 1 << 58  # the contract's largest row sum; three of them in a sum
    lab, col, conf = _dense(pn2, cuda, sp, sc, dp, 3, confidence=False)
    assert (lab == 4).all() and (col == [0, 128, 0]).all() and conf is None
    lab, col, conf = _dense(pn2, cuda, sp[:0], sc[:0], dp, 3)  # no sparse point at all
    assert (lab == -1).all() and not col.any() and (conf == 0).all()
    # the Python wrapper: the label form's argument checks, int64 scores only
    f = pn2.tf_ops.tf_interpolate.interpolate_scores_with_color
    T = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    sc = np.random.RandomState(0).randint(0, 1 << 32, (17, 9), dtype=np.int64)
    lab, col, conf = f(T(sp), T(sc), T(dp), 3)
    wl, wk, wc = S.interpolate_scores(sp, sc, dp, 3)
    assert np.array_equal(lab.cpu().numpy(), wl) and np.array_equal(col.cpu().numpy(), wk) and conf.cpu().numpy().tobytes() == wc.tobytes()
    assert lab.dtype == torch.int32 and col.dtype == torch.uint8 and conf.dtype == torch.float32
    for bad in (lambda: f(T(sp[:, :2]), T(sc), T(dp), 3), lambda: f(T(sp), T(sc[:5]), T(dp), 3), lambda: f(T(sp), T(sc), T(dp), 3.0),
                lambda: f(T(sp), T(sc), T(dp), 0), lambda: f(T(sp), T(sc), T(dp[:, :2]), 3)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        f(T(sp), T(sc.astype(np.int32)), T(dp), 3)


@pytest.mark.parametrize("kind", ["uniform", "duplicated"])
def test_interpolate_scores_agrees_with_the_label_kernel(pn2, cuda, kind):
    """every dense point, no exclusions.  One-hot scores with knn = 1 pick the nearest point's label; with two classes and an
    odd knn <= ns a strict majority always exists, so the first-maximal rule and the label form's running-count rule agree"""
    import torch
    sp, dp = _geometry(kind, 1000, 3000, seed=5)
    rs = np.random.RandomState(6)
    T = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    sl = rs.randint(0, 9, 1000).astype(np.int32)
    lab, col, _ = _dense(pn2, cuda, sp, np.eye(9, dtype=np.int64)[sl] * S.ONE, dp, 1)
    hl, hc = pn2.interpolate_label_with_color(T(sp), T(sl), T(dp), 1)
    assert np.array_equal(lab, hl.cpu().numpy()) and np.array_equal(col, hc.cpu().numpy())
    sl = rs.randint(0, 2, 1000).astype(np.int32)
    for knn in (1, 3, 5):
        lab, col, conf = _dense(pn2, cuda, sp, np.eye(2, dtype=np.int64)[sl] * S.ONE, dp, knn)
        hl, hc = pn2.interpolate_label_with_color(T(sp), T(sl), T(dp), knn)
        assert np.array_equal(lab, hl.cpu().numpy()) and np.array_equal(col, hc.cpu().numpy())
        assert set(np.unique(conf).tolist()) <= {np.float32(k / knn) for k in range(knn + 1)}


# ---- the flow ---------------------------------------------------------------------------------------------------------------
B, N, C = 4, 256, 9
NPOINT = dict(l1_npoint=128, l2_npoint=64, l3_npoint=32, l4_npoint=16)
PHASES = ((0.0, 0.0), (5.0, 5.0))


def _scene(n=3000, seed=7):
    """3000 points over 25 m x 15 m, float32 values; x distinct"""
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.permutation(n) * (25.0 / n), rs.uniform(0, 15, n), np.abs(rs.normal(0, 1.5, n))], 1).astype(np.float32).astype(np.float64)
    return pts, rs.randint(0, C, n).astype(np.int32), rs.randint(0, 256, (n, 3)) / 255.0


@pytest.fixture(scope="module")
def flow(pn2, cuda):
    """the predictor, the dataset, and one soft and one hard tiled prediction of the scene: made once, left unchanged"""
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.update(num_point=N, **NPOINT)
    predictor = pn2.predict.Predictor(None, C, hp, device=cuda, seed=5)
    pts, lab, col = _scene()
    ds = pn2.dataset.SemanticDataset(N, "validation", True, 10, 10, "", device=cuda, scenes=[(pts, lab, col, "s")])
    cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
    soft = pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=B, phases=PHASES, confusion=cm, vote="soft")
    assert set(predictor._score_graphs) == {(B, N)} and not predictor._graphs  # one graph shape, beside the label graphs
    hard = pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=B, phases=PHASES)
    assert set(predictor._score_graphs) == {(B, N)} and set(predictor._graphs) == {(B, N)}
    return dict(predictor=predictor, ds=ds, soft=soft, hard=hard, cm=cm)


def test_predict_scores_replays_what_it_captured(pn2, cuda, flow):
    import torch
    predictor = flow["predictor"]
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.rand((3, N, 6), generator=gen, dtype=torch.float32)  # a batch shape nobody has asked for yet
    x[:, :, 0:2] = x[:, :, 0:2] * 10 - 5
    x = x.to(cuda)
    assert (3, N) not in predictor._score_graphs
    first = predictor.predict_scores(x)
    assert (3, N) in predictor._score_graphs and (3, N) not in predictor._graphs
    again = predictor.predict_scores(x)
    assert first.dtype == torch.int32 and tuple(first.shape) == (3, N, C) and first.data_ptr() != again.data_ptr()
    assert torch.equal(first, again)
    kept = first.clone()
    other = predictor.predict_scores(x * 0.5)
    assert torch.equal(first, kept) and not torch.equal(other, first)  # a fresh tensor each time: a later call leaves it alone
    q = first.cpu().numpy().astype(np.int64)
    assert (q >= 0).all() and np.abs(q.sum(2) - S.ONE).max() <= C / 2 + 1 and len(np.unique(q.reshape(-1, C), axis=0)) > N
    # labels and scores of one forward pass: the labels are predict's; the probabilities are q * 2^-30
    pred, q2 = predictor.predict_labels_and_scores(x)
    assert torch.equal(q2, first) and torch.equal(pred, predictor.predict(x))
    assert (first.gather(2, pred.long().unsqueeze(2)).squeeze(2) == first.max(2).values).all()
    proba = predictor.predict_proba(x)
    assert proba.dtype == torch.float32 and torch.equal(proba, first.to(torch.float32) * 2.0 ** -30)
    with pytest.raises(ValueError):
        predictor.predict_scores(x[:, :, :3])


def test_predict_scene_tiled_soft_equals_the_replayed_loop(pn2, cuda, flow):
    import torch
    predictor, ds = flow["predictor"], flow["ds"]
    labels, scores = flow["soft"]
    n = len(ds.scene_points[0])
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (n,) and scores.dtype == torch.int64 and tuple(scores.shape) == (n, C)
    want = np.zeros((n, C), dtype=np.int64)
    batches = 0
    for ph in PHASES:
        cover = ds.tile_cover(0, ph, 1)
        assert cover.num_samples % B != 0  # the last batch is padded
        for q0 in range(0, cover.num_samples, B):
            data, sel, live = cover.batch(q0, B)
            q = predictor.predict_scores(data)
            assert S.vote_scores(want, sel.cpu().numpy(), live.cpu().numpy(), q.cpu().numpy()) == 0
            batches += 1
    assert batches > 2 * 2
    got = scores.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(labels.cpu().numpy(), np.argmax(want, 1)) and len(np.unique(want, axis=0)) > n // 2
    assert np.abs(want.sum(1) - len(PHASES) * S.ONE).max() <= C  # every point is covered once per phase
    g, p = ds.scene_labels[0].astype(np.int64), np.argmax(want, 1)
    assert np.array_equal(flow["cm"].confusion_matrix.reshape(-1), np.bincount(g * C + p, minlength=C * C))
    with pytest.raises(ValueError, match="vote"):
        pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=B, vote="mean")


def test_predict_scene_tiled_hard_is_what_it_was(pn2, cuda, flow):
    import torch
    predictor, ds = flow["predictor"], flow["ds"]
    labels, votes = flow["hard"]
    assert votes.dtype == torch.int32
    again = pn2.predict.predict_scene_tiled(predictor, ds, 0, batch_size=B, phases=PHASES, vote="hard")
    assert torch.equal(again[0], labels) and torch.equal(again[1], votes)
    predict = lambda data: predictor.predict(torch.from_numpy(data).to(cuda)).cpu().numpy()  # noqa: E731
    want_labels, want_votes = M.predict_scene(ds.scene_points[0], ds.scene_colors[0].astype(np.float32), 10, 10, N, C, predict, B,
                                              phases=PHASES)
    assert np.array_equal(votes.cpu().numpy(), want_votes) and np.array_equal(labels.cpu().numpy(), want_labels)
    assert (want_votes.sum(1) == 2).all()


def test_predict_scene_with_scores(pn2, cuda, flow):
    import torch
    predictor, ds = flow["predictor"], flow["ds"]
    points, labels, rows = pn2.predict.predict_scene(predictor, ds, 0, 6, batch_size=B, scores=True)  # batches of 4 and 2
    assert tuple(points.shape) == (6 * N, 3) and tuple(labels.shape) == (6 * N,) and tuple(rows.shape) == (6 * N, C)
    assert rows.dtype == torch.int32 and (rows >= 0).all()
    assert (rows.gather(1, labels.long().unsqueeze(1)).squeeze(1) == rows.max(1).values).all()
    assert ((rows.sum(1) - S.ONE).abs() <= C / 2 + 1).all()
    assert len(pn2.predict.predict_scene(predictor, ds, 0, 2, batch_size=B)) == 2


def test_label_dense_scores_does_not_depend_on_the_chunk(pn2, cuda, flow):
    import torch
    ds = flow["ds"]
    _, scores = flow["soft"]
    sp = torch.as_tensor(ds.scene_points[0]).to(cuda, torch.float32)
    rs = np.random.RandomState(4)
    dense = np.stack([rs.uniform(-1, 26, 5000), rs.uniform(-1, 16, 5000), rs.uniform(0, 4, 5000)], 1).astype(np.float32)
    truth = rs.randint(0, C, 5000).astype(np.int32)
    want = pn2.tf_ops.tf_interpolate.interpolate_scores_with_color(sp, scores, torch.from_numpy(dense).to(cuda), 3)
    wl, wk, wc = S.interpolate_scores(sp.cpu().numpy(), scores.cpu().numpy(), dense, 3)
    assert np.array_equal(want[0].cpu().numpy(), wl) and np.array_equal(want[1].cpu().numpy(), wk)
    assert want[2].cpu().numpy().tobytes() == wc.tobytes()
    for kw in (dict(), dict(chunk=5000), dict(chunk=1999)):
        cm = pn2.util.metric.ConfusionMatrix(C, device=cuda)
        got = pn2.predict.label_dense_scores(sp, scores, dense, truth, confusion=cm, **kw)
        for g, w in zip(got, want):
            assert torch.equal(g, w), kw
        assert np.array_equal(cm.confusion_matrix.reshape(-1), np.bincount(truth.astype(np.int64) * C + wl, minlength=C * C))
    # int32 score rows (predict_scene(scores=True)) are widened; numpy inputs are uploaded
    q32 = torch.clamp(scores, max=(1 << 31) - 1).to(torch.int32)
    a = pn2.predict.label_dense_scores(sp, q32, torch.from_numpy(dense).to(cuda))
    b = pn2.predict.label_dense_scores(sp.cpu().numpy(), q32.cpu().numpy().astype(np.int64), dense, chunk=3000)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        pn2.predict.label_dense_scores(sp, scores, dense, chunk=0)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tiled", [True, False])
def test_example_soft_route(pn2, cuda, tmp_path, tiled):
    U = pn2.util.point_cloud_util
    path = os.path.join(ROOT, "examples", "predict_semantic3d.py")
    flags = ["--soft", "--batch-size", str(B), "--points", str(N), "--npoint", "128,64,32,16", "--scenes", "1", "--scene-points", "20000",
             "--voxel", "0.1", "--chunk", "15000"]
    flags += ["--tiled", "--phases", "2"] if tiled else ["--num_samples", "6"]
    run = subprocess.run([sys.executable, path] + flags, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-3000:]
    assert "Soft vote: mean confidence" in out and "Sparse results" in out and "Global results" in out
    name = "syn_validation_0"
    dl = U.load_labels(str(tmp_path / "result" / "dense" / (name + ".labels")))
    sl = U.load_labels(str(tmp_path / "result" / "sparse" / (name + ".labels")))
    assert dl.shape == (20000,) and dl.min() >= 0 and dl.max() < 9 and sl.min() >= 0 and sl.max() < 9
    if not tiled:
        assert sl.shape == (6 * N,)
        return
    # the same scene, store and predictor in this process: the soft scores through to the dense labels
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("predict_semantic3d_example_soft", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    hp = dict(pn2.model.SEMANTIC_HYPERPARAMS)
    hp.setdefault("box_size_x", 10)
    hp.setdefault("box_size_y", 10)
    hp.update(use_color=1, num_point=N, **NPOINT)

    class Args:
        data, raw, set, scenes, scene_points, voxel, ingest = None, None, "validation", 1, 20000, 0.1, "host"
    ds, dense = ex.load_scenes(Args, hp, cuda)
    pred = pn2.predict.Predictor(None, ds.num_classes, hp, device=cuda)
    labels, scores = pn2.predict.predict_scene_tiled(pred, ds, 0, batch_size=B, phases=((0.0, 0.0), (5.0, 5.0)), vote="soft")
    assert np.array_equal(sl, labels.cpu().numpy())
    sp = torch.as_tensor(ds.scene_points[0]).to(cuda, torch.float32)
    lab, _, _ = pn2.predict.label_dense_scores(sp, scores, dense[name][0])
    assert np.array_equal(lab.cpu().numpy(), dl)
